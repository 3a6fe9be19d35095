// Front-end tables: psf's mel edges, the sparse per-lane mel decomposition of the float32 kernels, twiddles and DCT-II x lifter --
// built on the host in double precision, then rounded once to float32 -- the one device image kws_set_frontend uploads, and the
// host-only kws_host_* helpers of the CPU test-suite.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "kws_tables.h"

namespace kws {

static double hz2mel(double hz) { return 2595.0 * std::log10(1.0 + hz / 700.0); }
static double mel2hz(double mel) { return 700.0 * (std::pow(10.0, mel / 2595.0) - 1.0); }

// psf get_filterbanks: nfilt+2 points equally spaced in mel (numpy.linspace arithmetic: i*step + start,
// last point = stop), converted to FFT bins by floor((nfft+1)*hz/samplerate).
static void mel_edges(int nfilt, int nfft, int sample_rate, std::vector<int>& edges) {
    const double lowmel = hz2mel(0.0), highmel = hz2mel(sample_rate / 2.0);
    const int num = nfilt + 2;
    const double step = (highmel - lowmel) / (double)(num - 1);
    edges.resize(num);
    for (int i = 0; i < num; ++i) {
        volatile double prod = (double)i * step;  // two roundings, as numpy does (no fused multiply-add)
        double mel = prod + lowmel;
        if (i == num - 1) mel = highmel;
        edges[i] = (int)std::floor((nfft + 1) * mel2hz(mel) / sample_rate);
    }
}

static bool mel_edges_ok(const std::vector<int>& edges, int nfft) {
    for (size_t i = 0; i + 1 < edges.size(); ++i)
        if (edges[i + 1] < edges[i] || edges[i] < 0 || edges[i + 1] > nfft / 2) return false;
    return true;
}

// The sparse mel decomposition of the float32 kernels (FrontendTables::mel_*).
struct MelHost {
    std::vector<int> edges;            // nfilt+2
    std::vector<int> k0;               // 64
    std::vector<float> rw, fw;         // 8*64 each, [i][lane]
    std::vector<uint32_t> gather;      // 64
    std::vector<int> slot;             // nfft/2 (bin 256 belongs to no filter)
    std::vector<int> seg;              // 64
    int n_chunks = 0;
};

static bool build_mel_host(int nfilt, int nfft, int sample_rate, MelHost& out, std::string& err) {
    if (nfilt < 1 || nfilt > MAX_NFILT) {
        err = "nfilt must be in [1, 64]";
        return false;
    }
    mel_edges(nfilt, nfft, sample_rate, out.edges);
    if (!mel_edges_ok(out.edges, nfft)) {
        err = "mel edges are not monotone inside [0, nfft/2]";
        return false;
    }
    out.k0.assign(64, nfft / 2);
    out.rw.assign(MEL_CHUNK * 64, 0.f);
    out.fw.assign(MEL_CHUNK * 64, 0.f);
    out.gather.assign(64, 0u);
    out.slot.assign(nfft / 2, 0);
    std::vector<int> seg_first(nfilt + 2, 0), seg_count(nfilt + 2, 0);
    // segment s = bins [edge_s, edge_s+1): rising side of filter s (s < nfilt), falling side of filter s-1 (s >= 1);
    // it is cut into chunks of MEL_CHUNK bins, one chunk per lane, the chunks of a segment on adjacent lanes.
    int dense_lanes = 0;
    for (int s = 0; s <= nfilt; ++s) {
        seg_count[s] = (out.edges[s + 1] - out.edges[s] + MEL_CHUNK - 1) / MEL_CHUNK;
        dense_lanes += seg_count[s];
    }
    if (dense_lanes > 64) {
        err = "mel filterbank needs more than 64 chunks of 8 bins";
        return false;
    }
    // Lane layout: no segment straddles a 16-lane DPP row (idle lanes pad the rows), so the segmented sums can shift
    // with row_shl:1/2/4 fused into v_fmac_f32_dpp.  Every filterbank that fits 64 dense chunks at nfft = 512 and
    // the sample rates tried also fits this way (many filters = short segments); one that does not is refused.
    {
        int cursor = 0;
        for (int s = 0; s <= nfilt; ++s) {
            if (cursor % 16 + seg_count[s] > 16) cursor = (cursor + 15) / 16 * 16;
            seg_first[s] = cursor;
            cursor += seg_count[s];
            if (seg_count[s] > 8 || cursor > 64) {
                err = "mel filterbank does not fit 64 lanes with every segment (<= 8 chunks) inside one 16-lane row";
                return false;
            }
        }
    }
    int nchunks = 0;  // lanes in use (idle padding lanes included)
    for (int s = 0; s <= nfilt; ++s) {
        const int lo = out.edges[s], hi = out.edges[s + 1];
        int c = seg_first[s];
        for (int k0 = lo; k0 < hi; k0 += MEL_CHUNK, ++c) {
            out.k0[c] = k0;
            for (int i = 0; i < MEL_CHUNK && k0 + i < hi; ++i) out.slot[k0 + i] = MEL_STRIDE * c + i;
            for (int i = 0; i < MEL_CHUNK && k0 + i < hi; ++i) {
                const double k = k0 + i, width = (double)(hi - lo);
                if (s < nfilt) out.rw[i * 64 + c] = (float)((k - lo) / width);
                if (s >= 1) out.fw[i * 64 + c] = (float)((hi - k) / width);
            }
        }
        nchunks = std::max(nchunks, c);
    }
    // which neighbours (chunk + 1, + 2, + 4) share a chunk's segment: drives the in-register segmented sums
    out.seg.assign(64, 0);
    bool deep = false;
    for (int s = 0; s <= nfilt; ++s) {
        if (seg_count[s] > 8) {
            err = "a mel segment spans more than 8 chunks of 8 bins";
            return false;
        }
        deep = deep || seg_count[s] > 4;
        for (int i = 0; i < seg_count[s]; ++i)
            for (int d = 0; d < 3; ++d)
                if (i + (1 << d) < seg_count[s]) out.seg[seg_first[s] + i] |= 1 << d;
    }
    for (int c = 0; c < 64; ++c) out.seg[c] |= (deep ? 128 : 0) | 64;  // bit 6: row-safe layout (always)
    for (int j = 0; j < nfilt; ++j) {
        if (seg_count[j] > 255 || seg_count[j + 1] > 255) {
            err = "mel segment too long";
            return false;
        }
        out.gather[j] = (uint32_t)seg_first[j] | ((uint32_t)seg_count[j] << 8) | ((uint32_t)seg_first[j + 1] << 16) |
                        ((uint32_t)seg_count[j + 1] << 24);
    }
    out.n_chunks = nchunks;
    return true;
}

std::vector<double> build_twiddle64(int n) {
    std::vector<double> tw(2 * (size_t)n);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < n; ++k) {
        const double a = 2.0 * pi * k / n;
        tw[2 * k] = std::cos(a);
        tw[2 * k + 1] = -std::sin(a);
    }
    return tw;
}

// [numcep][nfilt]  DCT-II(ortho) x lifter
static std::vector<double> build_dct_lifter64(int nfilt, int numcep, int ceplifter) {
    std::vector<double> out((size_t)numcep * nfilt);
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < numcep; ++i) {
        const double lift = ceplifter > 0 ? 1.0 + (ceplifter / 2.0) * std::sin(pi * i / ceplifter) : 1.0;
        for (int j = 0; j < nfilt; ++j)
            out[(size_t)i * nfilt + j] = lift * (i == 0 ? std::sqrt(1.0 / nfilt) : std::sqrt(2.0 / nfilt) * std::cos(pi * i * (2 * j + 1) / (2.0 * nfilt)));
    }
    return out;
}

bool build_frontend_image(int sample_rate, int frame_len, int nfft, int nfilt, int numcep, int ceplifter, FrontendImage& im) {
    std::vector<int> edges;
    mel_edges(nfilt, nfft, sample_rate, edges);
    if (!mel_edges_ok(edges, nfft)) return false;
    // The float32 kernel is built for nfft = 512, frames of at most 512 samples and filterbanks its sparse lane layout can
    // hold; every other geometry runs on the float64 kernel (kws_mfcc_f64.hip).
    MelHost mel;
    std::string err;
    im.fast = nfft == NFFT && frame_len <= NFFT && build_mel_host(nfilt, nfft, sample_rate, mel, err) && mel.edges.front() == 0 &&
              mel.edges.back() == nfft / 2;
    if (!im.fast) {
        mel = MelHost();
        mel.k0.assign(64, 0);
        mel.rw.assign(MEL_CHUNK * 64, 0.f);
        mel.fw.assign(MEL_CHUNK * 64, 0.f);
        mel.gather.assign(64, 0u);
        mel.slot.assign(NFFT / 2, 0);
        mel.seg.assign(64, 0);
    }
    // float64 tables, and their float32 roundings: twiddles of the 512-point float32 kernel, DCT both dense and with rows
    // zero-padded to nfp floats
    const std::vector<double> tw64 = build_twiddle64(nfft), tw512 = build_twiddle64(NFFT), dct64 = build_dct_lifter64(nfilt, numcep, ceplifter);
    const std::vector<float> tw(tw512.begin(), tw512.end()), dct(dct64.begin(), dct64.end());
    const int nfp = (nfilt + 3) & ~3;
    std::vector<float> dct_pad(((size_t)numcep * nfp + 3) & ~(size_t)3, 0.f);
    for (int i = 0; i < numcep; ++i)
        for (int j = 0; j < nfilt; ++j) dct_pad[(size_t)i * nfp + j] = dct[(size_t)i * nfilt + j];
    // per-bin mel weights exactly as psf's get_filterbanks forms them (float64 divisions): bin i in [e_j, e_j+1) rises in
    // filter j with (i - e_j)/(e_j+1 - e_j) and falls in filter j-1 with (e_j+1 - i)/(e_j+1 - e_j)
    const int nb64 = nfft / 2 + 1;
    std::vector<double> melw(2 * (size_t)nb64, 0.0);
    for (int j = 0; j <= nfilt; ++j)
        for (int i = edges[j]; i < edges[j + 1]; ++i) {
            const double width = (double)(edges[j + 1] - edges[j]);
            melw[i] = (double)(i - edges[j]) / width;
            melw[(size_t)nb64 + i] = (double)(edges[j + 1] - i) / width;
        }

    size_t end = 0;
    auto place = [&](size_t& off, const auto& table) {  // the next 256-byte aligned offset
        off = end;
        end = (off + sizeof(table[0]) * table.size() + 255) & ~(size_t)255;
    };
    place(im.o_tw, tw), place(im.o_k0, mel.k0), place(im.o_rw, mel.rw), place(im.o_fw, mel.fw), place(im.o_g, mel.gather);
    place(im.o_dct, dct), place(im.o_slot, mel.slot), place(im.o_seg, mel.seg), place(im.o_tw64, tw64), place(im.o_edges, edges);
    place(im.o_dct64, dct64), place(im.o_melw, melw), place(im.o_dctp, dct_pad);
    im.bytes.assign(end, 0);
    auto put = [&](size_t off, const auto& table) { memcpy(&im.bytes[off], table.data(), sizeof(table[0]) * table.size()); };
    put(im.o_tw, tw), put(im.o_k0, mel.k0), put(im.o_rw, mel.rw), put(im.o_fw, mel.fw), put(im.o_g, mel.gather);
    put(im.o_dct, dct), put(im.o_slot, mel.slot), put(im.o_seg, mel.seg), put(im.o_tw64, tw64), put(im.o_edges, edges);
    put(im.o_dct64, dct64), put(im.o_melw, melw), put(im.o_dctp, dct_pad);
    return true;
}

FrontendTables FrontendImage::tables(const void* base) const {
    const unsigned char* b = static_cast<const unsigned char*>(base);
    FrontendTables t{};
    t.twiddle = reinterpret_cast<const float2*>(b + o_tw);
    t.mel_k0 = reinterpret_cast<const int*>(b + o_k0);
    t.mel_rw = reinterpret_cast<const float*>(b + o_rw);
    t.mel_fw = reinterpret_cast<const float*>(b + o_fw);
    t.mel_gather = reinterpret_cast<const uint32_t*>(b + o_g);
    t.dct = reinterpret_cast<const float*>(b + o_dct);
    t.mel_slot = reinterpret_cast<const int*>(b + o_slot);
    t.mel_seg = reinterpret_cast<const int*>(b + o_seg);
    t.tw64 = reinterpret_cast<const double*>(b + o_tw64);
    t.mel_edges = reinterpret_cast<const int*>(b + o_edges);
    t.dct64 = reinterpret_cast<const double*>(b + o_dct64);
    t.mel_w64 = reinterpret_cast<const double*>(b + o_melw);
    t.dct_pad = reinterpret_cast<const float*>(b + o_dctp);
    return t;
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_host_mel_edges(int nfilt, int nfft, int sample_rate, int* edges_out) {
    if (!edges_out || nfilt < 1 || nfft < 2 || sample_rate < 1) return KWS_EINVAL;
    std::vector<int> e;
    mel_edges(nfilt, nfft, sample_rate, e);
    memcpy(edges_out, e.data(), sizeof(int) * e.size());
    return KWS_OK;
}

int kws_host_mel_dense(int nfilt, int nfft, int sample_rate, float* fb_out) {
    if (!fb_out) return KWS_EINVAL;
    MelHost mel;
    std::string err;
    if (!build_mel_host(nfilt, nfft, sample_rate, mel, err)) return KWS_EUNSUPPORTED;
    const int nb = nfft / 2 + 1;
    std::fill(fb_out, fb_out + (size_t)nfilt * nb, 0.f);
    // expand exactly what the kernel evaluates: filter j = rising weights of its chunks + falling weights
    // of the next segment's chunks
    for (int j = 0; j < nfilt; ++j) {
        const uint32_t g = mel.gather[j];
        const int r0 = g & 255, nr = (g >> 8) & 255, q0 = (g >> 16) & 255, nq = g >> 24;
        for (int c = r0; c < r0 + nr; ++c)
            for (int i = 0; i < MEL_CHUNK; ++i) {
                const int k = mel.k0[c] + i;
                if (k < nb) fb_out[(size_t)j * nb + k] += mel.rw[i * 64 + c];
            }
        for (int c = q0; c < q0 + nq; ++c)
            for (int i = 0; i < MEL_CHUNK; ++i) {
                const int k = mel.k0[c] + i;
                if (k < nb) fb_out[(size_t)j * nb + k] += mel.fw[i * 64 + c];
            }
    }
    return KWS_OK;
}

int kws_host_mel_layout(int nfilt, int nfft, int sample_rate, int* first_lane_out, int* n_lanes_out, int* lanes_used, int* row_safe) {
    if (!first_lane_out || !n_lanes_out) return KWS_EINVAL;
    MelHost mel;
    std::string err;
    if (!build_mel_host(nfilt, nfft, sample_rate, mel, err)) return KWS_EUNSUPPORTED;
    // segment s = filter s's rising side; the last segment is the falling side of the last filter
    for (int j = 0; j < nfilt; ++j) {
        first_lane_out[j] = (int)(mel.gather[j] & 255);
        n_lanes_out[j] = (int)((mel.gather[j] >> 8) & 255);
    }
    first_lane_out[nfilt] = (int)((mel.gather[nfilt - 1] >> 16) & 255);
    n_lanes_out[nfilt] = (int)(mel.gather[nfilt - 1] >> 24);
    if (lanes_used) *lanes_used = mel.n_chunks;
    if (row_safe) *row_safe = (mel.seg[0] & 64) ? 1 : 0;
    return KWS_OK;
}

int kws_host_dct_lifter(int nfilt, int numcep, int ceplifter, float* out) {
    if (!out || nfilt < 1 || numcep < 1) return KWS_EINVAL;
    const std::vector<double> t = build_dct_lifter64(nfilt, numcep, ceplifter);
    std::copy(t.begin(), t.end(), out);  // the float32 table is the rounded float64 one
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
