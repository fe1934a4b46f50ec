// Steps 1-3 of the density-gradient tile (field_normal.hip's header comment), shared by field_grad_x_kernel and its backward
// (field_normal_bwd.hip): one definition, so the backward differentiates exactly the arithmetic the forward runs.
#pragma once
#include "mlp_device.hpp"

namespace perf {

// Fragment slots in LDS (16 B per lane each): the forward's A1[m][s] and Ao[s] as Layout<1, KS> numbers them, then
//   kA1P + s: A1T'[s]  row rho of the 32 x 32 result <-> input feature perm_in(rho), slot (h, j) <-> neuron slot_neuron(s, h, j)
//   kWoR + s: Wo[0][slot_neuron(s, h, j)], j = 0..7 -- the B operand of the pull-back before masking
// perm_in: D row rho = d_row(r, hh) is register r = (rho & 3) + 4 (rho >> 3) of half hh = (rho >> 2) & 1, and that register stands for
// feature r & 1 of level 8 (r >> 3) + 2 ((r >> 1) & 3) + hh.
__device__ __forceinline__ int perm_in(int rho) {
    const int hh = (rho >> 2) & 1, r = (rho & 3) + 4 * (rho >> 3);
    return 16 * (r >> 3) + 4 * ((r >> 1) & 3) + 2 * hh + (r & 1);
}

template <int KS>
struct GradXFrags {
    static constexpr int kA1P = Layout<1, KS>::n_fwd, kWoR = Layout<1, KS>::n_fwd + 4, n = Layout<1, KS>::n_fwd + 8;
};

// forward fragments + one pulled-back fragment pair per wave (blocks of four waves); the caller synchronises
template <int KS>
__device__ __forceinline__ void stage_grad_x_fragments(const uint16_t* __restrict__ w, u32x4* frag) {
    using L = Layout<1, KS>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    stage_fragments<1, KS, false>(w, frag);
    const int s = wave;
    const int fin = perm_in(c);
    uint16_t a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int nr = slot_neuron(s, h, j);
        a[j] = fin < L::n_in_pad ? w[L::w1_off + nr * L::n_in_pad + fin] : (uint16_t)0;
        b[j] = w[L::wo_off + nr];
    }
    frag[(GradXFrags<KS>::kA1P + s) * 64 + lane] = pack8(a);
    frag[(GradXFrags<KS>::kWoR + s) * 64 + lane] = pack8(b);
}

// ---- 1. features and their derivatives (per unit of the level's grid coordinate times scale = per unit of x01)
// b1: the packed first-layer operand; dF[2 * (4 s + i) + feature][axis]
template <typename T16, int KS>
__device__ __forceinline__ void features_and_derivatives(const GridParams& gp, const uint32_t* __restrict__ table, int n_levels, bool valid,
                                                         int h, float x, float y, float z, u32x4 (&b1)[KS], float (&dF)[8 * KS][3]) {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int level = 8 * s + 2 * i + h;
            const int q = 2 * (4 * s + i);
            uint32_t pair = 0u;
#pragma unroll
            for (int a = 0; a < 3; ++a) dF[q][a] = dF[q + 1][a] = 0.f;
            if (valid && level < n_levels) {
                const float scale = gp.scale[level];
                const Corners cr = corners_of(x, y, z, scale, gp.res[level], gp.size[level], gp.hashed[level] != 0);
                const uint32_t* t = table + gp.offset[level];
                uint32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t[cr.idx[k]];
                float wgt[8];
                corner_weights(cr.f, false, wgt);
                float v0[8], v1[8], a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {            // (encode_pair's sum, term for term)
                    v0[k] = T16::lo(v[k]); v1[k] = T16::hi(v[k]);
                    a0 = fmaf(wgt[k], v0[k], a0);
                    a1 = fmaf(wgt[k], v1[k], a1);
                }
                pair = T16::pack(a0, a1);
                const float fx = cr.f[0], fy = cr.f[1], fz = cr.f[2];
                const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
                float gx0 = 0.f, gx1 = 0.f, gy0 = 0.f, gy1 = 0.f, gz0 = 0.f, gz1 = 0.f;
#pragma unroll
                for (int p = 0; p < 4; ++p) {            // corner k = bit 0: x, bit 1: y, bit 2: z
                    const int a = p & 1, b = p >> 1;
                    const float wyz = wy[a] * wz[b], wxz = wx[a] * wz[b], wxy = wx[a] * wy[b];
                    const int kx = 2 * a + 4 * b, ky = a + 4 * b, kz = a + 2 * b;
                    gx0 = fmaf(wyz, v0[kx + 1] - v0[kx], gx0); gx1 = fmaf(wyz, v1[kx + 1] - v1[kx], gx1);
                    gy0 = fmaf(wxz, v0[ky + 2] - v0[ky], gy0); gy1 = fmaf(wxz, v1[ky + 2] - v1[ky], gy1);
                    gz0 = fmaf(wxy, v0[kz + 4] - v0[kz], gz0); gz1 = fmaf(wxy, v1[kz + 4] - v1[kz], gz1);
                }
                dF[q][0] = gx0 * scale; dF[q][1] = gy0 * scale; dF[q][2] = gz0 * scale;
                dF[q + 1][0] = gx1 * scale; dF[q + 1][1] = gy1 * scale; dF[q + 1][2] = gz1 * scale;
            }
            b1[s][i] = pair;
        }
}

// ---- 2. forward (mlp_fwd_kernel's, NH = 1) and 3. row 0 pulled back through the masks and W1^T
// hb: the packed post-ReLU activations (= the masks); dh: Wo[0][:] where the unit is active, as a B operand; o: the output tile;
// dx: register r of lane (c, h) is the derivative of the pre-activation w.r.t. the feature that lane formed in step 1
template <typename T16, int KS>
__device__ __forceinline__ void forward_and_pull_back(const u32x4* frag, int lane, const u32x4 (&b1)[KS], u32x4 (&hb)[4], u32x4 (&dh)[4],
                                                      f32x16& o, f32x16& dx) {
    using L = Layout<1, KS>;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        f32x16 acc = f32x16{0};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = T16::mfma(frag[(L::f_a1 + m * KS + s) * 64 + lane], b1[s], acc);
        relu_pack_plain<T16>(acc, hb[2 * m], hb[2 * m + 1]);
    }
    o = f32x16{0};
#pragma unroll
    for (int s = 0; s < 4; ++s) o = T16::mfma(frag[(L::f_ao + s) * 64 + lane], hb[s], o);
    dx = f32x16{0};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const u32x4 wo = frag[(GradXFrags<KS>::kWoR + s) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) dh[s][i] = wo[i] & nonzero_halves(hb[s][i]);
        dx = T16::mfma(frag[(GradXFrags<KS>::kA1P + s) * 64 + lane], dh[s], dx);
    }
}

}  // namespace perf
