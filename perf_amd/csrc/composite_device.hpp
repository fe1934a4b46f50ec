// The pieces of the packed-ray compositing arithmetic that the kernels of composite.hip share, each stated once: the team scans and sums,
// the weights of a sample, the distortion-loss term and the colour loss head.  Everything is __forceinline__ and keeps the association
// order of its expressions: kernels that share a piece give the same bits because they run the same code.  What is NOT here compiles to
// other code in at least one kernel when shared (profiles/composite_stated_once.json says which piece and how): the per-ray sums, the
// distortion-loss gradient and d sigma of the backward chunk, and the geometry loss head stay written out in their kernels.
#pragma once
#include "common.hpp"

namespace perf {

// ---- ray teams: W = 64, 16 or 4 lanes of a wavefront serve one ray (composite.hip: for_rays_of_wave), l = lane in the team --------
template <int W> struct Team { static constexpr int width = W; };

// The canonical scan: Kogge-Stone inside W-sample chunks with unfused adds, a carry between chunks (bit-exact against
// oracle/perf_oracle.py:packed_exclusive_sum_canonical; for <= W samples the offsets beyond W of a wider team only ever add exact zeros).
template <int W>
__device__ __forceinline__ float team_incl_scan_f(float x, int l) {
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        const float y = __shfl_up(x, off, W);
        if (l >= off) x = add_rn(x, y);
    }
    return x;
}
template <int W>
__device__ __forceinline__ float team_sum(float x) {
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, W);
    return x;
}
// exclusive prefix within the ray: returns ex for this lane's sample, updates carry
template <int W>
__device__ __forceinline__ float team_chunk_excl(float v, int l, float& carry) {
    const float inc = team_incl_scan_f<W>(v, l);
    float prev = __shfl_up(inc, 1, W);
    if (l == 0) prev = 0.f;
    const float ex = add_rn(carry, prev);
    carry = add_rn(carry, __shfl(inc, W - 1, W));
    return ex;
}
// inclusive suffix sum within the chunk (one value at a time: a helper that scans a pair packs the pair's adds into v_pk_add_f32)
template <int W>
__device__ __forceinline__ float team_suffix_incl(float x, int l) {
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        const float y = __shfl_down(x, off, W);
        if (l + off < W) x += y;
    }
    return x;
}
// ballot restricted to the caller's team (bit k = lane k of the team)
template <int W>
__device__ __forceinline__ unsigned long long team_ballot(bool p) {
    const unsigned long long b = __ballot(p);
    if (W == 64) return b;
    return (b >> (((threadIdx.x & 63) / W) * W)) & ((1ull << W) - 1ull);
}

// ---- a sample's T = exp(-ex), alpha = 1 - exp(-sd), w = T alpha from sd = sigma delta and ex, its canonical exclusive scan ------------
__device__ __forceinline__ void ray_weight(float ex, float sd, float& T, float& al, float& w) {
    T = expf(-ex);
    al = 1.0f - expf(-sd);
    w = T * al;
}

// ---- distortion loss, per ray:  sum_i ( d_i w_i^2 / 3 + 2 w_i (m_i W_i - WM_i) ),  W, WM exclusive prefixes.  Adds the term of this
// lane's sample to acc (w = m = d = 0 behind the ray's end)
template <int W>
__device__ __forceinline__ void distloss_chunk(float w, float m, float d, bool valid, int l, float& cW, float& cWM, float& acc) {
    const float Wp = team_chunk_excl<W>(w, l, cW);
    const float WMp = team_chunk_excl<W>(w * m, l, cWM);
    if (valid) acc += d * w * w * (1.0f / 3.0f) + 2.0f * w * (m * Wp - WMp);
}

// ---- loss heads (modules/scene/nerf.py:208-252 geometry, :281-293 colour; nerf_renderer.py:185-194 noise / background) ---------------
// smooth_l1(x, beta): 0.5 x^2 / beta for |x| < beta else |x| - 0.5 beta;  derivative x/beta or sign(x)
__device__ __forceinline__ float sl1(float x, float beta) { const float a = fabsf(x); return a < beta ? 0.5f * x * x / beta : a - 0.5f * beta; }
__device__ __forceinline__ float sl1_grad(float x, float beta) { return fabsf(x) < beta ? x / beta : (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)); }

// colour, one channel (app_loss_kernel runs a thread per channel, the ray head walks the three of its ray): colour' = colour +
// bg (1 - opacity), smooth-L1 at 5e-2 against gt; om = 1 - opacity, bg = 0 without a background
struct AppHead { float term, g; };                  // the channel's loss term, d loss / d colour
__device__ __forceinline__ AppHead app_head(float col, float bg, float om, float gt, float inv_n, float color_w, float loss_scale) {
    const float diff = col + bg * om - gt;
    return {sl1(diff, 5e-2f), sl1_grad(diff, 5e-2f) * inv_n * color_w * loss_scale};
}

}  // namespace perf
