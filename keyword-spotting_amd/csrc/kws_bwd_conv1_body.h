// The body of the conv1 backward kernels (kws_dscnn_bwd.hip), included once per kernel; the parameters are named da, a, x, T, F, H1,
// W1, nb, cpg, part.  The including kernel declares `constexpr bool MASK`: true = dZ1 = dA0 [A0 > 0] (kws_bwd_conv1_kernel), false =
// da is the finished dZ1 and a is not read (kws_bwd_conv1_dz_kernel, the train-mode BatchNorm path of kws_dscnn_bn.hip).  Textual
// inclusion for the reason kws_cnntrad_conv_body.h gives.
    __shared__ float s_dz[C1B_TP][65];
    __shared__ float s_b[4][64];
    const int tid = threadIdx.x, co = tid & 63, r0 = tid >> 6, g = blockIdx.x;
    const int P = H1 * W1;
    float acc[3][10];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[i][k] = 0.f;
    float bsum = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* dab = da + (size_t)b * 64 * P;
        const float* ab = a + (size_t)b * 64 * P;
        const float* xb = x + (size_t)b * T * F;
        for (int p0 = 0; p0 < P; p0 += C1B_TP) {
            for (int e = tid; e < 64 * C1B_TP; e += 256) {
                const int ch = e / C1B_TP, pp = e % C1B_TP, p = p0 + pp;
                float dz = 0.f;
                if (p < P && (!MASK || ab[(size_t)ch * P + p] > 0.f)) dz = dab[(size_t)ch * P + p];
                s_dz[pp][ch] = dz;
            }
            __syncthreads();
            const int n = min(C1B_TP, P - p0);
            for (int pp = 0; pp < n; ++pp) {
                const int p = p0 + pp, oh = p / W1, ow = p % W1;
                const float dz = s_dz[pp][co];
                if (r0 == 0) bsum += dz;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int kh = r0 + 4 * i;
                    const int ih = 2 * oh - 2 + kh;
                    if (kh < 10 && (unsigned)ih < (unsigned)T) {
                        const float* xr = xb + (size_t)ih * F;
#pragma unroll
                        for (int kw = 0; kw < 10; ++kw) {
                            const int iw = 2 * ow - 2 + kw;
                            if ((unsigned)iw < (unsigned)F) acc[i][kw] = fmaf(dz, xr[iw], acc[i][kw]);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    float* pg = part + (size_t)g * C1_PART;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int kh = r0 + 4 * i;
        if (kh < 10) {
#pragma unroll
            for (int kw = 0; kw < 10; ++kw) pg[co * DL::C1_TAPS + kh * 10 + kw] = acc[i][kw];
        }
    }
    s_b[r0][co] = bsum;
    __syncthreads();
    if (tid < 64) pg[DL::C1_W + tid] = s_b[0][tid];
