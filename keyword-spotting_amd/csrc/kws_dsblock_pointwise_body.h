// The body of the standalone block's pointwise kernels (kws_dsblock.hip), included once per kernel; the parameters are named dw,
// C_in, P, w, bias, C_out, Ho, Wo, pad, out.  The including kernel declares `constexpr bool RELU_OUT`: true = ReLU in the epilogue
// and a relu(bias) ring (kws_dsblock_pointwise_kernel), false = the pre-activation conv + bias with a ring equal to the bias (the
// train-mode BatchNorm path, kws_dscnn_bn.hip).  Textual inclusion, not a function, for the reason kws_cnntrad_conv_body.h gives: an
// always-inline body called from the kernel changes the existing kernel's instructions (tools/isa_diff.py).
    __shared__ float s_x[TK][TP + 1];
    __shared__ float s_w[TK][TC + 1];
    const int tid = threadIdx.x;
    const int b = blockIdx.z, p0 = blockIdx.x * TP, c0 = blockIdx.y * TC;
    const int tp = tid & 15, tc = tid >> 4;  // this thread: positions tp + 16 i, output channels tc + 16 j
    const int Hp = Ho + 2 * pad, Wp = Wo + 2 * pad;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const float* dwb = dw + (long)b * C_in * P;
    for (int k0 = 0; k0 < C_in; k0 += TK) {
        for (int e = tid; e < TK * TP; e += 256) {
            const int kk = e / TP, pp = e % TP;
            s_x[kk][pp] = (k0 + kk < C_in && p0 + pp < P) ? dwb[(long)(k0 + kk) * P + p0 + pp] : 0.f;
        }
        for (int e = tid; e < TK * TC; e += 256) {
            const int cc = e / TK, kk = e % TK;
            s_w[kk][cc] = (k0 + kk < C_in && c0 + cc < C_out) ? w[(long)(c0 + cc) * C_in + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TK; ++kk) {
            float xv[4], wv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = s_x[kk][tp + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) wv[j] = s_w[kk][tc + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(wv[j], xv[i], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = c0 + tc + 16 * j;
        if (co >= C_out) continue;
        const float bv = bias[co];
        float* op = out + ((long)b * C_out + co) * Hp * Wp;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = p0 + tp + 16 * i;
            if (p < P) op[(long)(p / Wo + pad) * Wp + (p % Wo) + pad] = RELU_OUT ? relu(acc[i][j] + bv) : acc[i][j] + bv;
        }
    }
    // the ring: the 1x1 convolution sees only zero padding there, so its value is relu(bias), or the bias; written once per
    // (batch, channel tile) by the workgroup of the first position tile
    if (pad > 0 && blockIdx.x == 0) {
        for (int cc = 0; cc < TC && c0 + cc < C_out; ++cc) {
            const float rv = RELU_OUT ? relu(bias[c0 + cc]) : bias[c0 + cc];
            float* op = out + ((long)b * C_out + c0 + cc) * Hp * Wp;
            for (int e = tid; e < Hp * Wp; e += 256) {
                const int h = e / Wp, x = e % Wp;
                if (h < pad || h >= Ho + pad || x < pad || x >= Wo + pad) op[e] = rv;
            }
        }
    }
