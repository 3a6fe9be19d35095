// The body of the composed path's conv1 kernels (kws_dsblock.hip), included once per kernel; the parameters are named x, C_in, T, F,
// wt, bias, Ho, Wo, out.  The including kernel declares `constexpr bool RELU_OUT`: true = ReLU in the epilogue
// (kws_conv1_any_kernel), false = the pre-activation conv1 + bias (the train-mode BatchNorm path, kws_dscnn_bn.hip).  Textual
// inclusion for the reason kws_cnntrad_conv_body.h gives.
    extern __shared__ float plane[];  // (T + 4) x (F + 4)
    const int tid = threadIdx.x, co = tid & 63, pg = tid >> 6;
    const int Hp = T + 4, Wp = F + 4, P = Ho * Wo, p0 = blockIdx.x * C1A_POS;
    float acc[C1A_PER];
    int base[C1A_PER];  // plane offset of the position's top-left tap (position p: rows 2*(p / Wo) .., columns 2*(p % Wo) ..)
#pragma unroll
    for (int k = 0; k < C1A_PER; ++k) {
        acc[k] = 0.f;
        const int p = min(p0 + pg + 4 * k, P - 1);
        base[k] = 2 * (p / Wo) * Wp + 2 * (p % Wo);
    }
    const float* xc = x + (size_t)blockIdx.y * C_in * T * F;
    for (int ci = 0; ci < C_in; ++ci) {
        __syncthreads();
        for (int i = tid; i < Hp * Wp; i += 256) {
            const int r = i / Wp - 2, c = i % Wp - 2;
            plane[i] = ((unsigned)r < (unsigned)T && (unsigned)c < (unsigned)F) ? xc[(size_t)ci * T * F + r * F + c] : 0.f;
        }
        __syncthreads();
        const float* wc = wt + (size_t)ci * 100 * 64 + co;
        for (int tap = 0; tap < 100; ++tap) {
            const float wv = wc[(size_t)tap * 64];
            const int off = (tap / 10) * Wp + tap % 10;
#pragma unroll
            for (int k = 0; k < C1A_PER; ++k) acc[k] = fmaf(wv, plane[base[k] + off], acc[k]);
        }
    }
    float* o = out + ((size_t)blockIdx.y * 64 + co) * P;
    const float bv = bias[co];
#pragma unroll
    for (int k = 0; k < C1A_PER; ++k) {
        const int p = p0 + pg + 4 * k;
        if (p < P) o[p] = RELU_OUT ? relu(acc[k] + bv) : acc[k] + bv;
    }
