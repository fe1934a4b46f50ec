// Density and its spatial gradient in ONE pass (perf_field_grad_x), and the per-ray normal composite (perf_normal_composite).
//
// n = -grad_x sigma / |grad_x sigma| is what a surface normal of a density field is.  The composed way to the gradient --
// perf_hashgrid_fwd -> perf_mlp_bwd(dfeat) -> perf_hashgrid_bwd_input -- writes and re-reads the fp32 feature gradient (128 B per
// sample at L = 16), forms a weight gradient nobody asked for, gathers the table twice and needs the fp32 table.  Here a wave owns a
// tile of 32 samples (mlp_device.hpp's forward, lane = (sample c, half h)):
//   1. lane (c, h) gathers the eight corners of ITS levels 8 s + 2 i + h ONCE and forms from them the packed feature pair -- the
//      arithmetic of encode_pair, so the forward is bit-identical to perf_field_infer's -- AND the pair's derivative along x, y, z
//      (derivative of the trilinear weights times the level's scale): 6 floats per level, kept in registers;
//   2. the 64-wide layer and the output layer run on MFMA as in mlp_fwd_kernel; the packed post-ReLU activations ARE the masks;
//   3. the output's row 0 is pulled back: dH = Wo[0][:] where the unit is active -- the 16-bit weights themselves, nothing is rounded --
//      and dF = W1^T dH is one more MFMA chain whose A rows are PERMUTED so that register r of lane (c, h) holds the derivative
//      w.r.t. exactly the feature (level 8 (r >> 3) + 2 ((r >> 1) & 3) + h, r & 1) that lane formed in step 1;
//   4. the contraction with the feature derivatives is in-lane, the two halves of a sample are added with one cross-half exchange,
//      and half 0 multiplies by the activation's derivative, the selector and 1 / (hi - lo) and stores 12 (+ 4) bytes.
// No feature gradient goes through memory, no weight gradient is formed.  Plain vector stores only.
//
// Built: tcnn table layout, Linear interpolation, one hidden layer, up to 16 levels, bf16 / fp16.  Everything else is refused.
#include "field_normal_device.hpp"

namespace perf {

struct GradXIn {
    GridParams gp;
    const uint32_t* table;
    const float* x01;
    float inv_extent[3];
};

template <typename T16, int KS>
__global__ __launch_bounds__(256) void field_grad_x_kernel(MlpParams mp, const uint16_t* __restrict__ w, const uint8_t* __restrict__ sel,
                                                           float* __restrict__ grad, float* __restrict__ sigma, int64_t n,
                                                           const int64_t* __restrict__ n_dev, GradXIn in) {
    const int64_t n_live = live_count(n, n_dev);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* frag = reinterpret_cast<u32x4*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    stage_grad_x_fragments<KS>(w, frag);
    __syncthreads();
    const int64_t n_tiles = (n_live + kTile - 1) / kTile;
    const int64_t tile_step = (int64_t)gridDim.x * 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += tile_step) {
        const int64_t si = tile * kTile + c;
        const bool valid = si < n_live;
        float x = 0.5f, y = 0.5f, z = 0.5f;
        if (valid) { x = in.x01[3 * si]; y = in.x01[3 * si + 1]; z = in.x01[3 * si + 2]; }
        // ---- 1.-3. (field_normal_device.hpp)
        u32x4 b1[KS], hb[4], dh[4];
        float dF[8 * KS][3];        // [2 * (4 s + i) + feature][axis]
        features_and_derivatives<T16, KS>(in.gp, in.table, mp.n_levels, valid, h, x, y, z, b1, dF);
        f32x16 o, dx;
        forward_and_pull_back<T16, KS>(frag, lane, b1, hb, dh, o, dx);
        // ---- 4. contract with the feature derivatives, add the two halves of the sample
        float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 8 * KS; ++r)
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] = fmaf(dx[r], dF[r][a], g[a]);
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] += __shfl_xor(g[a], 32);
        if (valid && h == 0) {          // (row 0 of the output is register 0 of half 0)
            const bool live = sel ? sel[si] != 0 : true;
            const float yv = o[0];
            float s_out, d_act;
            if (mp.out_act == PERF_ACT_SIGMOID) { s_out = 1.0f / (1.0f + expf(-yv)); d_act = s_out * (1.0f - s_out); }
            else if (mp.out_act == PERF_ACT_EXP) { s_out = expf(yv - mp.exp_shift); d_act = expf(fminf(yv - mp.exp_shift, 15.0f)); }
            else { s_out = yv; d_act = 1.0f; }
#pragma unroll
            for (int a = 0; a < 3; ++a) grad[3 * si + a] = live ? g[a] * d_act * in.inv_extent[a] : 0.f;
            if (sigma) sigma[si] = live ? s_out : 0.f;
        }
    }
}

// N[r] = sum_i w_i n_i over the ray's samples, n_i = -g_i / |g_i| (0 where g_i is 0 or not finite), then N / |N| (0 where |N| == 0):
// 16 lanes per ray -- a trained scene keeps a sample or two per ray -- summed in a fixed order (deterministic).
__global__ __launch_bounds__(256) void normal_composite_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                               const int32_t* __restrict__ packed, int64_t n_rays,
                                                               float* __restrict__ out) {
    const int sub = threadIdx.x & 15;
    const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool in_range = r < n_rays;
    const int64_t start = in_range ? packed[2 * r] : 0;
    const int cnt = in_range ? packed[2 * r + 1] : 0;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = sub; i < cnt; i += 16) {
        const float gx = g[3 * (start + i)], gy = g[3 * (start + i) + 1], gz = g[3 * (start + i) + 2];
        const float m = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
        if (m > 0.f && m <= 3.0e38f) {      // (scaled by the largest component first: |g|^2 of a trunc_exp gradient can leave fp32)
            const float ux = gx / m, uy = gy / m, uz = gz / m;
            const float k = -w[start + i] / sqrtf(ux * ux + uy * uy + uz * uz);
            a0 = fmaf(k, ux, a0); a1 = fmaf(k, uy, a1); a2 = fmaf(k, uz, a2);
        }
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) { a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); }
    if (in_range && sub == 0) {
        const float m = fmaxf(fabsf(a0), fmaxf(fabsf(a1), fabsf(a2)));
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (m > 0.f && m <= 3.0e38f) {
            const float ux = a0 / m, uy = a1 / m, uz = a2 / m;
            const float k = 1.0f / sqrtf(ux * ux + uy * uy + uz * uz);
            ox = ux * k; oy = uy * k; oz = uz * k;
        }
        out[3 * r] = ox; out[3 * r + 1] = oy; out[3 * r + 2] = oz;
    }
}

template <typename T16, int KS>
static void launch_grad_x(int blocks, hipStream_t st, MlpParams mp, const uint16_t* w, const uint8_t* sel, float* grad, float* sigma,
                          int64_t n, const int64_t* n_dev, const GradXIn& in) {
    constexpr int lds_bytes = GradXFrags<KS>::n * 1024;
    field_grad_x_kernel<T16, KS><<<dim3(blocks), dim3(256), lds_bytes, st>>>(mp, w, sel, grad, sigma, n, n_dev, in);
}

}  // namespace perf

using namespace perf;

extern "C" int perf_field_grad_x(const perf_grid_desc* grid, const perf_mlp_desc* mlp, const float* x01, const uint8_t* sel,
                                 const void* table16, const void* w16, const float* inv_extent, float* grad, float* sigma,
                                 int64_t n, const int64_t* n_dev, int dtype, void* stream) {
    PERF_REQUIRE(grid && mlp, "perf_field_grad_x: NULL descriptor");
    PERF_REQUIRE(n >= 0, "perf_field_grad_x: n < 0");
    PERF_REQUIRE(mlp->n_levels == grid->n_levels, "perf_field_grad_x: the MLP takes %d levels, the grid has %d", (int)mlp->n_levels, (int)grid->n_levels);
    PERF_REQUIRE(grid->layout == PERF_LAYOUT_TCNN, "perf_field_grad_x: tcnn table layout only (layout %d: the line-local layouts have no input gradient)", (int)grid->layout);
    PERF_REQUIRE(grid->interpolation == PERF_INTERP_LINEAR, "perf_field_grad_x: Linear interpolation only (Smoothstep is not built)");
    PERF_REQUIRE(grid->n_levels >= 1 && grid->n_levels <= 16, "perf_field_grad_x: 1..16 levels (%d: grids of more than 16 levels are not built)", (int)grid->n_levels);
    int nh, ks;
    int rc = check_mlp(mlp, &nh, &ks);
    if (rc) return rc;
    PERF_REQUIRE(nh == 1, "perf_field_grad_x: one hidden layer only (the density network); n_hidden_layers %d is not built", nh);
    PERF_REQUIRE(dtype == PERF_DTYPE_BF16 || dtype == PERF_DTYPE_FP16, "bad dtype %d", dtype);
    GradXIn in;
    rc = fill_params(grid, &in.gp);
    if (rc) return rc;
    if (n == 0) return PERF_OK;
    PERF_REQUIRE(x01 && table16 && w16, "perf_field_grad_x: NULL input pointer");
    PERF_REQUIRE(grad != nullptr, "perf_field_grad_x: NULL output pointer (grad)");
    in.table = (const uint32_t*)table16; in.x01 = x01;
    for (int a = 0; a < 3; ++a) in.inv_extent[a] = inv_extent ? inv_extent[a] : 1.0f;
    MlpParams mp{mlp->n_levels, mlp->n_out, mlp->out_act, mlp->exp_shift};
    const int blocks = mlp_blocks(n, 2);
    const hipStream_t st = as_stream(stream);
    if (dtype == PERF_DTYPE_BF16) {
        if (ks == 1) launch_grad_x<BF16, 1>(blocks, st, mp, (const uint16_t*)w16, sel, grad, sigma, n, n_dev, in);
        else launch_grad_x<BF16, 2>(blocks, st, mp, (const uint16_t*)w16, sel, grad, sigma, n, n_dev, in);
    } else {
        if (ks == 1) launch_grad_x<FP16, 1>(blocks, st, mp, (const uint16_t*)w16, sel, grad, sigma, n, n_dev, in);
        else launch_grad_x<FP16, 2>(blocks, st, mp, (const uint16_t*)w16, sel, grad, sigma, n, n_dev, in);
    }
    PERF_LAUNCH_CHECK("perf_field_grad_x");
    return PERF_OK;
}

extern "C" int perf_normal_composite(const float* weights, const float* grad, const int32_t* packed_info, int64_t n_rays,
                                     float* normal, void* stream) {
    PERF_REQUIRE(n_rays >= 0, "perf_normal_composite: n_rays < 0");
    if (n_rays == 0) return PERF_OK;
    PERF_REQUIRE(weights && grad && packed_info, "perf_normal_composite: NULL input pointer");
    PERF_REQUIRE(normal != nullptr, "perf_normal_composite: NULL output pointer");
    hipLaunchKernelGGL(normal_composite_kernel, dim3((unsigned)div_up(n_rays, 16)), dim3(256), 0, as_stream(stream), weights, grad,
                       packed_info, n_rays, normal);
    PERF_LAUNCH_CHECK("perf_normal_composite");
    return PERF_OK;
}
