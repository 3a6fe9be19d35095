// The body of the pointwise backward kernels (kws_dscnn_bwd.hip), included once per kernel; the parameters are named dy, dy_clip,
// dy_plane, dy_qstep, y, xdw, w, H, W, nb, cpg, dxdw, part.  The including kernel declares `constexpr bool MASK`: true = dZ = dY [Y > 0]
// (kws_bwd_pointwise_kernel), false = dy is the finished dZ and y is not read (kws_bwd_pointwise_dz_kernel, the train-mode BatchNorm
// path of kws_dscnn_bn.hip).  Textual inclusion for the reason kws_cnntrad_conv_body.h gives.
    __shared__ float s_w[64][65];        // W[co][ci]
    __shared__ float s_dz[64][PW_TP + 1];  // dZ[co][p]
    __shared__ float s_x[64][PW_TP + 1];   // X_dw[ci][p]
    __shared__ float s_b[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = blockIdx.x;
    const int P = H * W, Wq = W + 2, Q = (H + 2) * Wq;
    for (int e = tid; e < DL::PW_W; e += 256) s_w[e >> 6][e & 63] = w[e];
    __syncthreads();
    const int co0 = 32 * (wv >> 1), ci0 = 32 * (wv & 1), pt0 = 32 * (wv >> 1);
    // A operand of dX_dw = W^T dZ (32x32x2: A[i = l & 31][k = l >> 5]): A[ci][co] = W[co][ci], k-step s covers co 2s, 2s + 1
    float wa[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) wa[s] = s_w[2 * s + (lane >> 5)][ci0 + (lane & 31)];
    // the MFMA calls, zero fills and D rows stay spelled out in this kernel: through kws_train.h's mfma32 / zero16 / drow it
    // took 176 VGPRs for 168
    f32x16 gw;
#pragma unroll
    for (int r = 0; r < 16; ++r) gw[r] = 0.f;
    float bsum = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* dyb = dy + (size_t)b * dy_clip;
        const float* yb = y + (size_t)b * 64 * Q;
        const float* xb = xdw + (size_t)b * 64 * P;
        {
            const float* yc = yb + (size_t)lane * Q;
            const float* dc = dyb + (size_t)lane * dy_plane;
            for (int r0 = wv; r0 < Q; r0 += 4 * RUN) {  // runs of RUN positions, each summed from zero
                const int r1 = min(Q, r0 + 4 * RUN);
                float t = 0.f;
                for (int q = r0; q < r1; q += 4)
                    if (!MASK || yc[q] > 0.f) t += dc[(size_t)q * dy_qstep];
                bsum += t;
            }
        }
        for (int p0 = 0; p0 < P; p0 += PW_TP) {
            for (int e = tid; e < 64 * PW_TP; e += 256) {
                const int row = e / PW_TP, pp = e % PW_TP, p = p0 + pp;
                float dz = 0.f, xv = 0.f;
                if (p < P) {
                    const int q = (p / W + 1) * Wq + p % W + 1;
                    if constexpr (MASK) {
                        const float yv = yb[(size_t)row * Q + q];
                        dz = yv > 0.f ? dyb[(size_t)row * dy_plane + (size_t)q * dy_qstep] : 0.f;
                    } else {
                        dz = dyb[(size_t)row * dy_plane + (size_t)q * dy_qstep];
                    }
                    xv = xb[(size_t)row * P + p];
                }
                s_dz[row][pp] = dz;
                s_x[row][pp] = xv;
            }
            __syncthreads();
            // g_pw_w: A[i = co][k = p] = dZ, B[k = p][j = ci] = X_dw (32x32x2: lane l holds k = l >> 5); the tile's sum starts
            // from zero and is added to the running one, so no f32 chain runs longer than 64 positions
            f32x16 gt;
#pragma unroll
            for (int r = 0; r < 16; ++r) gt[r] = 0.f;
#pragma unroll
            for (int s = 0; s < PW_TP / 2; ++s) {
                const float a = s_dz[co0 + (lane & 31)][2 * s + (lane >> 5)];
                const float bb = s_x[ci0 + (lane & 31)][2 * s + (lane >> 5)];
                gt = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, gt, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) gw[r] += gt[r];
            // dX_dw: B[k = co][j = p] = dZ
            f32x16 d;
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 32; ++s) d = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[s], s_dz[2 * s + (lane >> 5)][pt0 + (lane & 31)], d, 0, 0, 0);
            // C/D: col = l & 31 (position), row = (r & 3) + 8 (r >> 2) + 4 (l >> 5) (input channel)
            const int p = p0 + pt0 + (lane & 31);
            if (p < P) {
                float* o = dxdw + (size_t)b * 64 * P + (size_t)ci0 * P + p;
#pragma unroll
                for (int r = 0; r < 16; ++r) o[(size_t)((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * P] = d[r];
            }
            __syncthreads();
        }
    }
    float* pg = part + (size_t)g * PW_PART;
    // C/D of 32x32: col = l & 31 (ci), row = (r & 3) + 8 (r >> 2) + 4 (l >> 5) (co)
#pragma unroll
    for (int r = 0; r < 16; ++r) pg[(co0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 64 + ci0 + (lane & 31)] = gw[r];
    s_b[wv][lane] = bsum;
    __syncthreads();
    if (tid < 64) pg[DL::PW_W + tid] = (s_b[0][tid] + s_b[1][tid]) + (s_b[2][tid] + s_b[3][tid]);
