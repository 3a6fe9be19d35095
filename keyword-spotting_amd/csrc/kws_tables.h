// Front-end tables (kws_tables.hip), built on the host in double and rounded once to float32: what kws_set_frontend and
// kws_spec_f32 upload.  Host code only; no context.
#pragma once
#include <vector>

#include "kws_internal.h"

namespace kws {

std::vector<double> build_twiddle64(int n);  // [n][2]  (cos, -sin)(2*pi*k/n)
// The one allocation behind FrontendTables, every table 256-byte aligned, and where each table lies in it.
struct FrontendImage {
    std::vector<unsigned char> bytes;
    size_t o_tw, o_k0, o_rw, o_fw, o_g, o_dct, o_slot, o_seg, o_tw64, o_edges, o_dct64, o_melw, o_dctp;
    bool fast;  // the float32 kernel covers this geometry (nfft 512, frame_len <= 512, sparse mel layout fits)
    FrontendTables tables(const void* base) const;
};
// false: the mel edges are not monotone inside [0, nfft/2]
bool build_frontend_image(int sample_rate, int frame_len, int nfft, int nfilt, int numcep, int ceplifter, FrontendImage& out);

}  // namespace kws
