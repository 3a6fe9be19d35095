// The body of the cnn-trad-fpool3 conv kernels (kws_cnntrad.hip), included once per feature source inside a kernel template
// <bool H2> whose parameters are named w, conv_out and clip_scale.  The including kernel defines
//   CT_SOURCE_PROLOGUE   statements that declare `int clip` (the workspace slot this workgroup writes), leave the kernel when the
//                        workgroup is past the launch's count, and declare whatever CT_FEAT reads
//   CT_FEAT(i)           float i (row-major, 0 .. 989) of this workgroup's 99 x 10 map
// and undefines both after the include.  The map is read in ONE place, the staging loop; everything after it is per clip, so
// every source yields the bits of the same rows handed over as a contiguous clip.  (Textual inclusion, not a function: an
// always-inline body called from the kernels changes the instruction selection of the two batch kernels, tools/isa_diff.py.)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t m0_bits;
    float* xp = reinterpret_cast<float*>(smem);
    unsigned char* planes = smem + XP_BYTES;
    constexpr int NP = H2 ? 2 : 3;  // operand pieces
    unsigned char* win = planes + NP * PLANE_BYTES;  // H2: conv1's pre-split input windows, [piece][padded row][start column][8 x f16]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31;
    CT_SOURCE_PROLOGUE

    // ---- stage: zero-padded input map, zero regions of the pooled planes ---------------------------------
    for (int i = tid; i < XP_H * XP_W; i += CT_NT) xp[i] = 0.f;
    if (tid < NP * PL_ZERO_BYTES / 4)
        reinterpret_cast<uint32_t*>(planes + (tid / (PL_ZERO_BYTES / 4)) * PLANE_BYTES + PL_ZERO_OFF)[tid % (PL_ZERO_BYTES / 4)] = 0u;
    if (tid == 0) m0_bits = 0u;
    __syncthreads();
    // H2: per-clip scales.  post1 / post2 take a layer's accumulators back to true units, s1 maps the pooled conv1 output
    // into f16's range (see the note at split_pair)
    float post1 = 1.f, post2 = 1.f, s1 = 1.f;
    if constexpr (H2) {
        float v[2] = {0.f, 0.f}, mx = 0.f;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int i = tid + n * CT_NT;
            if (i < CT_T * CT_F) {
                v[n] = CT_FEAT(i);
                mx = fmaxf(mx, fabsf(v[n]));
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        if (lane == 0) atomicMax(&m0_bits, __builtin_bit_cast(uint32_t, mx));  // non-negative floats order like their bits
        __syncthreads();
        const float m0 = __builtin_bit_cast(float, m0_bits);
        const int k0 = pow2_exp_for(m0);
        const float bound1 = (w.w1_abs * m0 + w.b1_max) * 1.001f;
        const float bound2 = (w.w2_abs * bound1 + w.b2_max) * 1.001f;
        const int k1 = pow2_exp_for(bound1), k2 = pow2_exp_for(bound2);
        post1 = pow2f(-k0) * w.inv_sw1;
        s1 = pow2f(k1);
        post2 = pow2f(-k1) * w.inv_sw2;
        if (tid == 0) clip_scale[clip] = pow2f(k2);
        const float s0 = pow2f(k0);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int i = tid + n * CT_NT;
            if (i < CT_T * CT_F) xp[(i / CT_F + 9) * XP_W + i % CT_F + 3] = v[n] * s0;
        }
        __syncthreads();
        // conv1's B operands, split ONCE: window (padded row r, start column f) = the eight consecutive scaled inputs a lane
        // needs for one kernel row, as one 16-byte hi and one 16-byte lo' fragment.  (Gathered and split per use it was
        // 8 LDS reads + ~30 VALU instructions per three MFMAs, and conv1 took more than a third of the kernel.)
        for (int i = tid; i < XP_H * CT_F; i += CT_NT) {
            const float* src = xp + (i / CT_F) * XP_W + i % CT_F;
            const float y[8] = {src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7]};
            uintx4 hi, lo;
            split2(y, hi, lo);
            *reinterpret_cast<uintx4*>(win + i * 16) = hi;
            *reinterpret_cast<uintx4*>(win + i * 16 + WIN_PLANE_BYTES) = lo;
        }
    } else {
        for (int i = tid; i < CT_T * CT_F; i += CT_NT)
            xp[(i / CT_F + 9) * XP_W + i % CT_F + 3] = CT_FEAT(i);
    }
    __syncthreads();

    // ---- conv1 + ReLU + frequency max-pool -> pre-split planes ------------------------------------------
    // A tile = 3 time rows x 10 bins in columns 0..29.  k-block kb covers kernel rows 2kb (lanes 0..31) and 2kb+1
    // (lanes 32..63), all 8 kernel columns: the lane's eight B elements are consecutive floats of one padded row.
    // Wavefront w owns channel tile w & 1 and keeps that tile's 30 pre-split A fragments (120 registers) for the
    // whole phase -- streamed per tile they would cost 2 MB of L1 traffic per clip -- and walks tiles w>>1, +4, ...
    {
        const int ct = wv & 1;
        uintx4 af[CT_K1H / 2][NP];  // [k-block][piece]
        {
            const uintx4* asrc = reinterpret_cast<const uintx4*>(H2 ? w.c1_h2 : w.c1_split) + ct * (NP * 64) + lane;
#pragma unroll
            for (int kb = 0; kb < CT_K1H / 2; ++kb)
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) af[kb][pc] = asrc[(kb * 2 * NP + pc) * 64];
        }
        float bias[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bias[r] = w.c1_b[ct * 32 + row_of(r, half)] * s1;  // H2: in the planes' scale (s1 = 1 otherwise)
        const float ps1 = post1 * s1;
        const int cc = col < 30 ? col : 29;
        const int tr = cc / CT_F, f = cc % CT_F;
        const bool owner = col < 30 && f % 3 == 0 && f < 9;
#ifdef KWS_X_CT_NO_CONV1  // timing ablation: no conv1 (the planes keep whatever LDS held)
        for (int u = C1_TILES; u < C1_TILES; u += CT_NW / 2) {
#else
        for (int u = wv >> 1; u < C1_TILES; u += CT_NW / 2) {
#endif
            const int t = 3 * u + tr;
            const float* base = xp + (t + half) * XP_W + f;
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc2 = acc;  // two chains, summed below
            if constexpr (H2) {
                // B operand = the pre-split window (padded row t + 2kb + half, start column f): two aligned ds_read_b128 per
                // k-block, no VALU work; fetched two k-blocks ahead.  acc = hi * hi, acc2 = the cross terms (units of 2^-11)
                const unsigned char* wb = win + ((t + half) * CT_F + f) * 16;
                uintx4 bq[3][2];
                auto wload = [&](int kb, uintx4 (&d)[2]) {
                    d[0] = *reinterpret_cast<const uintx4*>(wb + kb * (2 * CT_F * 16));
                    d[1] = *reinterpret_cast<const uintx4*>(wb + kb * (2 * CT_F * 16) + WIN_PLANE_BYTES);
                };
                wload(0, bq[0]);
                wload(1, bq[1]);
#pragma unroll
                for (int kb = 0; kb < CT_K1H / 2; ++kb) {
                    if (kb + 2 < CT_K1H / 2) wload(kb + 2, bq[(kb + 2) % 3]);
#ifdef KWS_X_CT_NO_C1_MFMA  // timing ablation: conv1's loads and epilogue without the matrix instructions
                    acc[kb] += __builtin_bit_cast(float, bq[kb % 3][0][0] ^ bq[kb % 3][1][1] ^ af[kb][0][0] ^ af[kb][NP - 1][1]);
#else
                    acc2 = mfma_f16(af[kb][0], bq[kb % 3][1], acc2);
                    acc = mfma_f16(af[kb][0], bq[kb % 3][0], acc);
                    acc2 = mfma_f16(af[kb][NP - 1], bq[kb % 3][0], acc2);
#endif
                }
            } else {
                float y[2][8];
                auto gather = [&](int kb, float (&dst)[8]) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) dst[j] = base[kb * 2 * XP_W + j];
                };
                gather(0, y[0]);
                gather(1, y[1]);
#pragma unroll
                for (int kb = 0; kb < CT_K1H / 2; ++kb) {
                    const int cur = kb & 1;
                    uintx4 bh, bm, bl;
                    split3(y[cur], bh, bm, bl);
                    if (kb + 2 < CT_K1H / 2) gather(kb + 2, y[cur]);
                    // six piece products, smallest first
                    acc = mfma_bf16(af[kb][NP - 1], bh, acc);
                    acc2 = mfma_bf16(af[kb][0], bl, acc2);
                    acc = mfma_bf16(af[kb][1], bm, acc);
                    acc2 = mfma_bf16(af[kb][1], bh, acc2);
                    acc = mfma_bf16(af[kb][0], bm, acc);
                    acc2 = mfma_bf16(af[kb][0], bh, acc2);
                }
            }
            if constexpr (!H2) acc += acc2;
            // bias, ReLU, max over bins (f, f+1, f+2) via two lane shifts; lanes with f in {0,3,6} own a pooled value
            const int p = t * CT_FP + f / 3;
#ifdef KWS_X_CT_NO_C1_EPILOGUE  // timing ablation: conv1 without its epilogue (one store keeps the accumulators alive)
            if (acc[0] + acc[5] + acc[10] + acc[15] == 12345.f) planes[p] = 1;
            continue;
#endif
            if constexpr (H2) {
                // relu(x * post + b) * s1 is monotone in x, so the pool runs on the raw sums (two DPP maxima per value) and the
                // affine map, with s1 folded in (powers of two: exact), once on the maximum -- same bits as pooling afterwards
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    float m[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float v = acc[r + e] + acc2[r + e] * LO_UNSCALE;
                        const float a = fmaxf(v, lane_up(v));
                        m[e] = relu(fmaxf(a, lane_up(a)) * ps1 + bias[r + e]);
                    }
                    if (owner) {  // channels co, co+1 (co even) as one dword per piece
                        const int co = ct * 32 + row_of(r, half);
                        uint32_t* dst = reinterpret_cast<uint32_t*>(planes + p * PL_STRIDE + co * 2);
                        uint32_t hi, lo;
                        split_pair(m[0], m[1], hi, lo);
                        dst[0] = hi;
                        dst[PLANE_BYTES / 4] = lo;
                    }
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                float m[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float v = relu(acc[r + e] + bias[r + e]);
                    const float a = lane_up(v), b = lane_up(a);
                    m[e] = fmaxf(v, fmaxf(a, b));
                }
                if (owner) {  // channels co, co+1 (co even) as one dword per piece
                    const int co = ct * 32 + row_of(r, half);
                    uint32_t* dst = reinterpret_cast<uint32_t*>(planes + p * PL_STRIDE + co * 2);
                    const float r0 = m[0] - top16(m[0]), r1 = m[1] - top16(m[1]);
                    dst[0] = pack_top16(m[0], m[1]);
                    dst[PLANE_BYTES / 4] = pack_top16(r0, r1);
                    dst[(NP - 1) * PLANE_BYTES / 4] = pack_top16(r0 - top16(r0), r1 - top16(r1));
                }
            }
        }
    }
    __syncthreads();

    // ---- conv2 + ReLU -> HBM ------------------------------------------------------------------------------
    // K = 2560 ordered (kh, kw, cin): k-block (kk = kh*4 + kw, cb) covers input channels 16cb..16cb+15 of the input
    // position (t + kh - 4, fp + kw - 1); lane (column, half) reads its eight channels 16cb + 8half .. +7 of each
    // piece with one ds_read_b128.  One unit per wavefront, a single round: wavefront w takes channel tile w & 1 and
    // a group of position tiles -- {0,1,2}, {3,4,5}, {6,7}, {8,9} for w >> 1 = 0..3 -- so that the two wavefronts of
    // a SIMD (w, w+4) carry 3 + 2 tiles, the same on every SIMD, and the A operands (983 KB of pre-split weights
    // streaming from L2 through L1, which would otherwise be as busy as the matrix pipe) are fetched once per
    // k-block for all of the wavefront's tiles.
    auto conv2_unit = [&](auto ntile_tag, int tile0) {
        constexpr int NTILE = decltype(ntile_tag)::value;
        constexpr int NACC = H2 ? 2 : 1;       // H2: [0] = hi * hi, [1] = cross terms in units of 2^-11
        constexpr int NPROD = H2 ? 3 : 6;      // piece products per k-block
        const int ct = wv & 1;
        int p[NTILE], t[NTILE], fp[NTILE];
        bool pvalid[NTILE];
        floatx16 acc[NTILE][NACC];
#pragma unroll
        for (int i = 0; i < NTILE; ++i) {
            p[i] = (tile0 + i) * 32 + col;
            pvalid[i] = p[i] < CT_P2;
            t[i] = p[i] / CT_FP;  // columns past the map keep their natural geometry: they read zeros from their own bank slot
            fp[i] = p[i] % CT_FP;
#pragma unroll
            for (int a = 0; a < NACC; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][a][r] = 0.f;
        }
        const uintx4* asrc = reinterpret_cast<const uintx4*>(H2 ? w.c2_h2 : w.c2_split) + ct * (NP * 64) + lane;
        // Pipeline at k-block granularity: the A operands of (kk+1, cb) are requested right after those of (kk, cb)
        // have been used (four k-blocks ahead of their use, an L2 round trip); the B operands of the next k-block
        // are read from LDS one k-block ahead.
        uintx4 af[4][NP];         // [cb][piece] of this wavefront's channel tile
        uintx4 bf[2][NTILE][NP];  // [parity of the k-block][tile][piece]
        auto a_index = [&](int kk, int cb, int pc2) { return (((size_t)kk * 4 + cb) * 2 * NP + pc2) * 64; };
        auto a_load = [&](int kk, int cb) {
#pragma unroll
            for (int pc2 = 0; pc2 < NP; ++pc2) af[cb][pc2] = asrc[a_index(kk, cb, pc2)];
        };
        auto b_addr = [&](int kk, int i) -> const unsigned char* {
            const int kh = kk >> 2, kw = kk & 3;
            const int tin = t[i] + kh - 4, fin = fp[i] + kw - 1;
            const bool ok = pvalid[i] && (unsigned)tin < (unsigned)CT_T && (unsigned)fin < (unsigned)CT_FP;
            const int natural = (tin * CT_FP + fin) * PL_STRIDE + half * 16;  // may lie outside the plane
            return planes + (ok ? natural : PL_ZERO_OFF + (natural & 255));
        };
        auto b_load = [&](const unsigned char* const (&ba)[NTILE], int cb, uintx4 (&dst)[NTILE][NP]) {
#pragma unroll
            for (int i = 0; i < NTILE; ++i)
#pragma unroll
                for (int pc2 = 0; pc2 < NP; ++pc2) dst[i][pc2] = *reinterpret_cast<const uintx4*>(ba[i] + cb * 32 + pc2 * PLANE_BYTES);
        };
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) a_load(0, cb);
        const unsigned char* ba[NTILE];
#pragma unroll
        for (int i = 0; i < NTILE; ++i) ba[i] = b_addr(0, i);
        b_load(ba, 0, bf[0]);
#ifdef KWS_X_CT_NO_CONV2  // timing ablation: no conv2 loop
        for (int kk = CT_K2H * CT_K2W; kk < CT_K2H * CT_K2W; ++kk) {
#else
        for (int kk = 0; kk < CT_K2H * CT_K2W; ++kk) {
#endif
            const unsigned char* ba_next[NTILE];
#pragma unroll
            for (int i = 0; i < NTILE; ++i) ba_next[i] = b_addr(kk + 1 < CT_K2H * CT_K2W ? kk + 1 : kk, i);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int cur = cb & 1;
                const bool more = kk + 1 < CT_K2H * CT_K2W;
                // The loads of the next k-block are spread between the MFMAs (one load behind each matrix
                // instruction, pinned with scheduling barriers): issued in a lump after them, the matrix pipe drains
                // while the wavefront works through a dozen memory instructions.  An A piece is re-requested for
                // (kk+1, cb) right behind its last use.
#pragma unroll
                for (int q = 0; q < NPROD; ++q) {  // piece products, smallest first, tiles interleaved
                    // three-way bf16: (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi); f16 pair: (hi,lo') (hi,hi) (lo',hi)
                    const int pa = H2 ? (q == 2 ? 1 : 0) : (q == 0 ? 2 : (q == 2 || q == 3) ? 1 : 0);
                    const int pb = H2 ? (q == 0 ? 1 : 0) : ((q == 0 || q == 3 || q == 5) ? 0 : (q == 1 ? 2 : 1));
                    const int dst = H2 ? (q == 1 ? 0 : 1) : 0;
#pragma unroll
                    for (int i = 0; i < NTILE; ++i) {
                        if constexpr (H2)
                            acc[i][dst] = mfma_f16(af[cb][pa], bf[cur][i][pb], acc[i][dst]);
                        else
                            acc[i][dst] = mfma_bf16(af[cb][pa], bf[cur][i][pb], acc[i][dst]);
                        __builtin_amdgcn_sched_barrier(0);
                        const int n = q * NTILE + i;  // one B load (tile n / NP, piece n % NP) of the next k-block per MFMA
#ifdef KWS_X_CT_NO_BLOAD  // timing ablation: B operands are not refreshed
                        if (n < 0) {
#else
                        if (n < NP * NTILE) {
#endif
                            const unsigned char* src = (cb < 3 ? ba[n / NP] + (cb + 1) * 32 : ba_next[n / NP]) + (n % NP) * PLANE_BYTES;
                            bf[cur ^ 1][n / NP][n % NP] = *reinterpret_cast<const uintx4*>(src);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    // last use of an A piece: three-way lo after product 0, mid after 3, hi after 5; pair hi after 1, lo' after 2
                    const int done = H2 ? (q == 1 ? 0 : (q == 2 ? 1 : -1)) : (q == 0 ? 2 : (q == 3 ? 1 : (q == 5 ? 0 : -1)));
#ifdef KWS_X_CT_NO_ALOAD  // timing ablation: A operands are not refreshed
                    if (false) {
#else
                    if (more && done >= 0) {
#endif
                        af[cb][done] = asrc[a_index(kk + 1, cb, done)];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NTILE; ++i) ba[i] = ba_next[i];
        }
#pragma unroll
        for (int i = 0; i < NTILE; ++i) {
            if (pvalid[i]) {
                float* o = conv_out + (size_t)clip * (CH * CT_P2) + p[i];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * 32 + row_of(r, half);
                    float v = acc[i][0][r];
                    if constexpr (H2) v = (v + acc[i][NACC - 1][r] * LO_UNSCALE) * post2;
                    o[co * CT_P2] = relu(v + w.c2_b[co]);
                }
            }
        }
    };
    {
        const int g = wv >> 1;
        if (g < 2)
            conv2_unit(std::integral_constant<int, 3>{}, 3 * g);
        else
            conv2_unit(std::integral_constant<int, 2>{}, 6 + 2 * (g - 2));
    }
