// The sphere distance field (include/perf_hip_sphere.h): a Smoothstep hash grid over directions, a 35 -> 64 -> 64 -> 1 fp32 MLP with
// Softplus(beta = 100), the gradient of its output with respect to the direction, and the backward of both with respect to the
// parameters.  Two kernels; everything is fp32, nothing is rounded to a 16-bit type.
//
// A wave owns a tile of 32 samples; sample c of the tile lives in the two lanes c and c + 32 (h = lane >> 5), as in the density
// kernels.  Every matrix product runs on the exact fp32 MFMA (32x32x2: lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31], one register each; bitwise an fmaf chain) with M = neurons, N = samples:
//   * the D layout of a product (lane (c, h), block m, register r  <->  neuron nrn(m, r, h) = 32 m + 8 (r >> 2) + 4 h + (r & 3) of
//     sample c) IS the B operand of the next product, k-step (m, t = r): the reduction runs over the neurons in that order and the
//     A operand -- a weight -- is read from LDS at the matching column.  No activation is transposed between layers; the activations
//     apply register by register.
//   * the weights are staged once per workgroup, row-major with an odd pitch (W1: 37, W2: 65), so that ONE copy serves the product and
//     its transpose (the pull-back) without bank conflicts inside a half wave.
//   * a lane encodes the eight levels 2 q + h of its sample (register 2 q + e = feature e of level 2 q + h); the feature rows of the
//     transposed first layer are permuted so that a lane gets back the adjoints of exactly the features it formed: J^T (.) is in-lane.
//   * the direction's three inputs take two more k-steps of the first layer ((u0, u1), (u2, -)); their pull-back A^T d1 is 96 fmaf per
//     lane on the vector unit.
// Backward: beside (z1, z2) a tangent (z1d, z2d) along c = dL/dg is carried -- c . g = -w3 . h2d -- and the adjoints of (raw, tangent)
// = (a, 1) are pulled back together (the header states the recurrences).  The weight gradients are products over the SAMPLES: the
// two operands go through a wave-private LDS tile [sample][neuron] (pitch 68: 16-byte stores from the D layout, conflict-free
// transposing reads), K = 32 samples = 16 k-steps, accumulators across tiles in registers (dW2: 64, dW1's feature columns: 32).  The
// bias sums and the three direction columns of dW1 are column sums of the A operand the lane loads anyway: in-lane fmaf, 12
// registers.  Compiler's register and scratch report: DESIGN.md 5.5.1.
//
// Network part: tile t goes to wave (t / 256) % 4 of workgroup t % 256 -- a FIXED grid of 256 workgroups, whatever n -- the four waves
// are added in a fixed order, the 256 partials by mlp_reduce_block in a fixed order (db3 = -sum a, one number, from the upstream itself in double): deterministic, and samples appended with a
// zero upstream add zeros to the same sums.  Table part: the lane that formed a level's features recomputes corners and weights and
// scatters with fp32 global atomics into the zero-filled table part (last bits depend on the order the atomics retire in).
// Plain vector loads and stores and vector atomics only.
#include "grid_device.hpp"
#include "mlp_reduce_device.hpp"
#include "../../include/perf_hip_sphere.h"

namespace perf {

constexpr int kSphTile = 32;            // samples per wave tile
constexpr int kP1 = 37, kP2 = 65;       // LDS pitches of W1 (64 x 35) and W2 (64 x 64)
constexpr int kPT = 68;                 // pitch of a transposition tile [32 samples][64 (+4) values]
constexpr int kSphBwdBlocks = 256;      // the backward's grid, and the number of partials: fixed
constexpr int kW1s = 0, kW2s = kW1s + 64 * kP1, kB1s = kW2s + 64 * kP2, kB2s = kB1s + 64, kW3s = kB2s + 64, kNetLds = kW3s + 64;
static_assert(kNetLds % 4 == 0, "the tiles behind the weights must start 16-byte aligned");
constexpr int kSphFwdLds = kNetLds * 4;
constexpr int kSphBwdLds = (kNetLds + 4 * 2 * kSphTile * kPT) * 4;

struct SphNet { int n_in, w1, b1, w2, b2, w3, b3, n_net; };
__host__ __device__ __forceinline__ SphNet sph_net(int n_levels) {
    SphNet s;
    s.n_in = 3 + 2 * n_levels;
    s.w1 = 0; s.b1 = 64 * s.n_in; s.w2 = s.b1 + 64; s.b2 = s.w2 + 64 * 64; s.w3 = s.b2 + 64; s.b3 = s.w3 + 64; s.n_net = s.b3 + 1;
    return s;
}

__device__ __forceinline__ int nrn(int m, int r, int h) { return 32 * m + 8 * (r >> 2) + 4 * h + (r & 3); }
// column of W1 that feature register t of half h multiplies (level 2 (t >> 1) + h, feature t & 1)
__device__ __forceinline__ int fcol(int t, int h) { return 3 + 2 * (2 * (t >> 1) + h) + (t & 1); }
// keeps the scheduler from hoisting a whole product's LDS reads (or a whole sample's gathers) above it: the registers they would hold are
// the accumulators'
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// torch's Softplus(beta = 100, threshold = 20) and its two derivatives
__device__ __forceinline__ float sp0(float z) { const float t = 100.0f * z; return t > 20.0f ? z : log1pf(expf(t)) / 100.0f; }
__device__ __forceinline__ float sp1(float z) { const float t = 100.0f * z; if (t > 20.0f) return 1.0f; const float e = expf(t); return e / (e + 1.0f); }
__device__ __forceinline__ void sp12(float z, float& d1, float& d2) {
    const float t = 100.0f * z;
    if (t > 20.0f) { d1 = 1.0f; d2 = 0.f; return; }
    const float e = expf(t), q = 1.0f / (e + 1.0f);
    d1 = e * q; d2 = 100.0f * (e * q) * q;
}

__device__ __forceinline__ void stage_net(const float* __restrict__ net, const SphNet& s, float* lds) {
    for (int i = threadIdx.x; i < 64 * kP1; i += blockDim.x) { const int r = i / kP1, c = i - r * kP1; lds[kW1s + i] = c < s.n_in ? net[s.w1 + r * s.n_in + c] : 0.f; }
    for (int i = threadIdx.x; i < 64 * kP2; i += blockDim.x) { const int r = i / kP2, c = i - r * kP2; lds[kW2s + i] = c < 64 ? net[s.w2 + r * 64 + c] : 0.f; }
    for (int i = threadIdx.x; i < 64; i += blockDim.x) { lds[kB1s + i] = net[s.b1 + i]; lds[kB2s + i] = net[s.b2 + i]; lds[kW3s + i] = net[s.w3 + i]; }
}

// ---- the encoding of one lane: features (and, kJ, their derivatives with respect to x) of the levels 2 q + h ------------------------
template <bool kJ>
__device__ __forceinline__ void encode_lane(const GridParams& gp, const float2* __restrict__ table, bool live, int h, float x, float y, float z,
                                            float feat[16], float J[16][3]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int l = 2 * q + h;
        float f0 = 0.f, f1 = 0.f, j0[3] = {0.f, 0.f, 0.f}, j1[3] = {0.f, 0.f, 0.f};
        if (live && l < gp.n_levels) {
            const float scale = gp.scale[l];
            const Corners c = corners_of(x, y, z, scale, gp.res[l], gp.size[l], gp.hashed[l] != 0);
            const float2* t = table + gp.offset[l];
            float2 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = t[c.idx[k]];
            float s[3], d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { const float f = c.f[a]; s[a] = f * f * (3.0f - 2.0f * f); d[a] = 6.0f * f * (1.0f - f) * scale; }
            const float wx[2] = {1.0f - s[0], s[0]}, wy[2] = {1.0f - s[1], s[1]}, wz[2] = {1.0f - s[2], s[2]};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
                const float w = (wx[bx] * wy[by]) * wz[bz];
                f0 = fmaf(w, v[k].x, f0); f1 = fmaf(w, v[k].y, f1);
                if constexpr (kJ) {
                    const float g[3] = {(bx ? d[0] : -d[0]) * (wy[by] * wz[bz]), (by ? d[1] : -d[1]) * (wx[bx] * wz[bz]), (bz ? d[2] : -d[2]) * (wx[bx] * wy[by])};
#pragma unroll
                    for (int a = 0; a < 3; ++a) { j0[a] = fmaf(g[a], v[k].x, j0[a]); j1[a] = fmaf(g[a], v[k].y, j1[a]); }
                }
            }
        }
        if ((q & 3) == 3) sched_fence();
        feat[2 * q] = f0; feat[2 * q + 1] = f1;
        if constexpr (kJ) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { J[2 * q][a] = j0[a]; J[2 * q + 1][a] = j1[a]; }
        }
    }
}

// ---- the four products of the chain.  i = lane & 31 and k = lane >> 5 index the A operand; the same two numbers are (c, h) of B and D
template <bool kBias>
__device__ __forceinline__ void layer1(const float* lds, int i, int k, const float feat[16], float u01, float u2z, f32x16 z[2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[m][r] = kBias ? lds[kB1s + nrn(m, r, k)] : 0.f;
    const float* w = lds + kW1s + i * kP1;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int col = fcol(t, k);
        z[0] = mfma32(w[col], feat[t], z[0]);
        z[1] = mfma32(w[32 * kP1 + col], feat[t], z[1]);
        if ((t & 3) == 3) sched_fence();
    }
    z[0] = mfma32(w[k], u01, z[0]);
    z[1] = mfma32(w[32 * kP1 + k], u01, z[1]);
    z[0] = mfma32(k ? 0.f : w[2], u2z, z[0]);
    z[1] = mfma32(k ? 0.f : w[32 * kP1 + 2], u2z, z[1]);
}

template <bool kBias>
__device__ __forceinline__ void layer2(const float* lds, int i, int k, const f32x16 hin[2], f32x16 z[2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[m][r] = kBias ? lds[kB2s + nrn(m, r, k)] : 0.f;
    const float* w = lds + kW2s + i * kP2;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = nrn(m, t, k);
            z[0] = mfma32(w[col], hin[m][t], z[0]);
            z[1] = mfma32(w[32 * kP2 + col], hin[m][t], z[1]);
            if ((t & 3) == 3) sched_fence();
        }
}

// out = W2^T din
__device__ __forceinline__ void layer2_t(const float* lds, int i, int k, const f32x16 din[2], f32x16 out[2]) {
    out[0] = f32x16{0}; out[1] = f32x16{0};
    const float* w = lds + kW2s + i;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = nrn(m, t, k) * kP2;
            out[0] = mfma32(w[row], din[m][t], out[0]);
            out[1] = mfma32(w[row + 32], din[m][t], out[1]);
            if ((t & 3) == 3) sched_fence();
        }
}

// out[r] = (B^T din) at this lane's feature register r (W1 = [A | B]); row i of the product is feature register ((i >> 3) << 2) | (i & 3)
// of half (i >> 2) & 1 -- the inverse of the D layout's row 8 (r >> 2) + 4 h + (r & 3)
__device__ __forceinline__ void layer1_t(const float* lds, int i, int k, const f32x16 din[2], f32x16& out) {
    out = f32x16{0};
    const float* w = lds + kW1s + fcol(((i >> 3) << 2) | (i & 3), (i >> 2) & 1);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            out = mfma32(w[nrn(m, t, k) * kP1], din[m][t], out);
            if ((t & 7) == 7) sched_fence();
        }
}

// =================================================================== forward ==========================================================
template <bool kGrad>
__global__ __launch_bounds__(256, 2) void sphere_field_fwd_kernel(GridParams gp, const float2* __restrict__ table, const float* __restrict__ net,
                                                                   const float* __restrict__ dirs, float* __restrict__ raw, float* __restrict__ grad,
                                                                   int64_t n) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SphNet s = sph_net(gp.n_levels);
    stage_net(net, s, lds);
    __syncthreads();
    const float b3 = net[s.b3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (n + kSphTile - 1) / kSphTile;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t si = tile * kSphTile + c;
        const bool live = si < n;
        float u[3] = {0.f, 0.f, 0.f};
        if (live) { u[0] = dirs[3 * si]; u[1] = dirs[3 * si + 1]; u[2] = dirs[3 * si + 2]; }
        const float x = u[0] * 0.49f + 0.49f, y = u[1] * 0.49f + 0.49f, z = u[2] * 0.49f + 0.49f;         // (two roundings, as torch forms it)
        float feat[16], J[16][3];
        encode_lane<kGrad>(gp, table, live, h, x, y, z, feat, J);
        f32x16 z1[2], z2[2], h1[2];
        layer1<true>(lds, c, h, feat, h ? u[1] : u[0], h ? 0.f : u[2], z1);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) h1[m][r] = sp0(z1[m][r]);
        layer2<true>(lds, c, h, h1, z2);
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc = fmaf(lds[kW3s + nrn(m, r, h)], sp0(z2[m][r]), acc);
        acc += __shfl_xor(acc, 32);
        if (live && h == 0) raw[si] = -(acc + b3);
        if constexpr (kGrad) {
            f32x16 d2[2], d1[2], ft;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) d2[m][r] = sp1(z2[m][r]) * lds[kW3s + nrn(m, r, h)];
            layer2_t(lds, c, h, d2, d1);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) d1[m][r] *= sp1(z1[m][r]);
            layer1_t(lds, c, h, d1, ft);
            float g[3] = {0.f, 0.f, 0.f}, gx[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* w = lds + kW1s + nrn(m, r, h) * kP1;
#pragma unroll
                    for (int a = 0; a < 3; ++a) g[a] = fmaf(w[a], d1[m][r], g[a]);
                }
#pragma unroll
            for (int t = 0; t < 16; ++t)
#pragma unroll
                for (int a = 0; a < 3; ++a) gx[a] = fmaf(J[t][a], ft[t], gx[a]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float v = fmaf(0.49f, gx[a], g[a]);
                v += __shfl_xor(v, 32);
                if (live && h == 0) grad[3 * si + a] = -v;
            }
        }
    }
}

// =================================================================== backward =========================================================
struct SphBwdAcc {
    f32x16 w2[2][2];        // [mo][no][r]: dW2[32 mo + 8 (r >> 2) + 4 k + (r & 3)][32 no + j]
    f32x16 w1[2];           // [mo][r]: the same rows, feature column j = 16 h' + t of the B tile
    float a[2][3];          // [mo][a]: direction column a of dW1, row 32 mo + i, this lane's sample parity k
    float b1[2], b2[2], w3[2];
};
constexpr int kSphAccRegs = 64 + 32 + 6 + 6;

// accumulator q of kSphAccRegs (q is a constant after unrolling)
__device__ __forceinline__ float acc_get(const SphBwdAcc& A, int q) {
    if (q < 64) return A.w2[q >> 5][(q >> 4) & 1][q & 15];
    q -= 64;
    if (q < 32) return A.w1[q >> 4][q & 15];
    q -= 32;
    if (q < 6) return A.a[q / 3][q % 3];
    q -= 6;
    if (q < 2) return A.b1[q];
    if (q < 4) return A.b2[q - 2];
    return A.w3[q - 4];
}
__device__ __forceinline__ void acc_add(SphBwdAcc& A, int q, float v) {
    if (q < 64) { A.w2[q >> 5][(q >> 4) & 1][q & 15] += v; return; }
    q -= 64;
    if (q < 32) { A.w1[q >> 4][q & 15] += v; return; }
    q -= 32;
    if (q < 6) { A.a[q / 3][q % 3] += v; return; }
    q -= 6;
    if (q < 2) A.b1[q] += v;
    else if (q < 4) A.b2[q - 2] += v;
    else A.w3[q - 4] += v;
}

// the 16-byte stores of a lane's D-layout values into its sample's row of a tile
__device__ __forceinline__ void tile_put(float* t, int c, int h, const f32x16 v[2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(t + c * kPT + 32 * m + 8 * g + 4 * h) = f32x4{v[m][4 * g], v[m][4 * g + 1], v[m][4 * g + 2], v[m][4 * g + 3]};
}

// the B tile of the first layer's products: columns 16 h + t = feature register t of half h, columns 32..34 = the direction part
__device__ __forceinline__ void tile_put_input(float* t, int c, int h, const float f[16], const float u[3]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(t + c * kPT + 16 * h + 4 * g) = f32x4{f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3]};
    if (h == 0) *reinterpret_cast<f32x4*>(t + c * kPT + 32) = f32x4{u[0], u[1], u[2], 0.f};
}

__global__ __launch_bounds__(256, 1) void sphere_field_bwd_kernel(GridParams gp, const float2* __restrict__ table, const float* __restrict__ net,
                                                                   const float* __restrict__ dirs, const float* __restrict__ draw,
                                                                   const float* __restrict__ dgrad, float* __restrict__ partials,
                                                                   float* __restrict__ gtable, int64_t n) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SphNet s = sph_net(gp.n_levels);
    stage_net(net, s, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    float* tA = lds + kNetLds + wave * (2 * kSphTile * kPT);
    float* tB = tA + kSphTile * kPT;
    SphBwdAcc A;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        A.w2[m][0] = f32x16{0}; A.w2[m][1] = f32x16{0}; A.w1[m] = f32x16{0};
        A.a[m][0] = A.a[m][1] = A.a[m][2] = 0.f; A.b1[m] = A.b2[m] = A.w3[m] = 0.f;
    }
    const int64_t n_tiles = (n + kSphTile - 1) / kSphTile;
    for (int64_t tile = (int64_t)blockIdx.x + (int64_t)kSphBwdBlocks * wave; tile < n_tiles; tile += (int64_t)kSphBwdBlocks * 4) {
        const int64_t si = tile * kSphTile + c;
        const bool live = si < n;
        float u[3] = {0.f, 0.f, 0.f}, cd[3] = {0.f, 0.f, 0.f}, a_up = 0.f;
        if (live) {
            u[0] = dirs[3 * si]; u[1] = dirs[3 * si + 1]; u[2] = dirs[3 * si + 2];
            if (draw) a_up = draw[si];
            if (dgrad) { cd[0] = dgrad[3 * si]; cd[1] = dgrad[3 * si + 1]; cd[2] = dgrad[3 * si + 2]; }
        }
        const float x = u[0] * 0.49f + 0.49f, y = u[1] * 0.49f + 0.49f, z = u[2] * 0.49f + 0.49f;
        const float xd[3] = {0.49f * cd[0], 0.49f * cd[1], 0.49f * cd[2]};
        // ---- 1. features and their tangent fd = J xd
        float feat[16], fd[16];
        {
            float J[16][3];
            encode_lane<true>(gp, table, live, h, x, y, z, feat, J);
#pragma unroll
            for (int t = 0; t < 16; ++t) fd[t] = fmaf(J[t][2], xd[2], fmaf(J[t][1], xd[1], J[t][0] * xd[0]));
        }
        // ---- 2. the forward and its tangent
        f32x16 z1[2], z1d[2], z2[2], z2d[2], h1[2], h1d[2];
        layer1<true>(lds, c, h, feat, h ? u[1] : u[0], h ? 0.f : u[2], z1);
        layer1<false>(lds, c, h, fd, h ? cd[1] : cd[0], h ? 0.f : cd[2], z1d);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) { h1[m][r] = sp0(z1[m][r]); h1d[m][r] = sp1(z1[m][r]) * z1d[m][r]; }
        layer2<true>(lds, c, h, h1, z2);
        layer2<false>(lds, c, h, h1d, z2d);
        // ---- 3. adjoints at the second layer: z2t = z2~, z2dt = z2d~ (they take the registers of z2, z2d); q = the summand of dw3
        {
            f32x16 q[2];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float zz = z2[m][r], w3 = lds[kW3s + nrn(m, r, h)];
                    float d1, d2;
                    sp12(zz, d1, d2);
                    const float h2d = d1 * z2d[m][r];
                    q[m][r] = -fmaf(a_up, sp0(zz), h2d);
                    z2[m][r] = d1 * (-a_up * w3) + d2 * z2d[m][r] * (-w3);
                    z2d[m][r] = d1 * (-w3);
                }
            __builtin_amdgcn_wave_barrier();
            tile_put(tA, c, h, q);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 0; t < 16; ++t) { const float* row = tA + (2 * t + h) * kPT + c; A.w3[0] += row[0]; A.w3[1] += row[32]; }
        }
        // ---- 4. dW2 += z2~ (x) h1 + z2d~ (x) h1d,  db2 += z2~
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            __builtin_amdgcn_wave_barrier();
            tile_put(tA, c, h, round == 0 ? z2 : z2d);
            tile_put(tB, c, h, round == 0 ? h1 : h1d);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float* ra = tA + (2 * t + h) * kPT + c;
                const float* rb = tB + (2 * t + h) * kPT + c;
                const float a0 = ra[0], a1 = ra[32], b0 = rb[0], b1 = rb[32];
                A.w2[0][0] = mfma32(a0, b0, A.w2[0][0]); A.w2[0][1] = mfma32(a0, b1, A.w2[0][1]);
                A.w2[1][0] = mfma32(a1, b0, A.w2[1][0]); A.w2[1][1] = mfma32(a1, b1, A.w2[1][1]);
                if (round == 0) { A.b2[0] += a0; A.b2[1] += a1; }
                if ((t & 3) == 3) sched_fence();
            }
        }
        // ---- 5. back through W2, adjoints at the first layer (in the registers of h1, h1d)
        layer2_t(lds, c, h, z2, h1);
        layer2_t(lds, c, h, z2d, h1d);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float d1, d2;
                sp12(z1[m][r], d1, d2);
                h1[m][r] = d1 * h1[m][r] + d2 * z1d[m][r] * h1d[m][r];          // z1~
                h1d[m][r] = d1 * h1d[m][r];                                     // z1d~
            }
        // ---- 6. dW1 += z1~ (x) [u; f] + z1d~ (x) [c; fd],  db1 += z1~
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            __builtin_amdgcn_wave_barrier();
            tile_put(tA, c, h, round == 0 ? h1 : h1d);
            tile_put_input(tB, c, h, round == 0 ? feat : fd, round == 0 ? u : cd);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float* ra = tA + (2 * t + h) * kPT + c;
                const float* rb = tB + (2 * t + h) * kPT;
                const float a0 = ra[0], a1 = ra[32], b0 = rb[c];
                A.w1[0] = mfma32(a0, b0, A.w1[0]);
                A.w1[1] = mfma32(a1, b0, A.w1[1]);
#pragma unroll
                for (int a = 0; a < 3; ++a) { const float ua = rb[32 + a]; A.a[0][a] = fmaf(a0, ua, A.a[0][a]); A.a[1][a] = fmaf(a1, ua, A.a[1][a]); }
                if (round == 0) { A.b1[0] += a0; A.b1[1] += a1; }
                if ((t & 3) == 3) sched_fence();
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 7. the table part: d table[idx_k(l)] += w_k f~_l + (grad_x w_k . xd) fd~_l
        f32x16 ft, fdt;
        layer1_t(lds, c, h, h1, ft);
        layer1_t(lds, c, h, h1d, fdt);
        // (a sample without an upstream has f~ = fd~ = 0: its 128 atomics of zero are not issued; the network part does not depend on this)
        if (live && (a_up != 0.f || cd[0] != 0.f || cd[1] != 0.f || cd[2] != 0.f)) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int l = 2 * q + h;
                if (l >= gp.n_levels) continue;
                const float p0 = ft[2 * q], p1 = ft[2 * q + 1], pd0 = fdt[2 * q], pd1 = fdt[2 * q + 1];
                const float scale = gp.scale[l];
                const uint32_t size = gp.size[l];
                const Corners cr = corners_of(x, y, z, scale, gp.res[l], size, gp.hashed[l] != 0);
                float sm[3], d[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) { const float f = cr.f[a]; sm[a] = f * f * (3.0f - 2.0f * f); d[a] = 6.0f * f * (1.0f - f) * scale * xd[a]; }
                const float wx[2] = {1.0f - sm[0], sm[0]}, wy[2] = {1.0f - sm[1], sm[1]}, wz[2] = {1.0f - sm[2], sm[2]};
                float* t = gtable + 2 * gp.offset[l];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
                    const float w = (wx[bx] * wy[by]) * wz[bz];
                    const float dw = fmaf(bz ? d[2] : -d[2], wx[bx] * wy[by], fmaf(by ? d[1] : -d[1], wx[bx] * wz[bz], (bx ? d[0] : -d[0]) * (wy[by] * wz[bz])));
                    const uint32_t idx = cr.idx[k];
                    if (idx < size) {                       // (corners_of keeps the indices inside the level)
                        unsafeAtomicAdd(t + 2 * (uint64_t)idx, fmaf(dw, pd0, w * p0));
                        unsafeAtomicAdd(t + 2 * (uint64_t)idx + 1, fmaf(dw, pd1, w * p1));
                    }
                }
            }
        }
    }
    // ---- the four waves' accumulators, added in a fixed order through LDS (lane-linear slots behind the weights); ONE partial per workgroup
    __syncthreads();
    float* red = lds + kNetLds;
    static_assert(kSphAccRegs * 64 <= 4 * 2 * kSphTile * kPT, "reduction scratch exceeds the tiles");
    for (int src = 1; src < 4; ++src) {
        if (wave == src) {
#pragma unroll
            for (int q = 0; q < kSphAccRegs; ++q) red[q * 64 + lane] = acc_get(A, q);
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < kSphAccRegs; ++q) acc_add(A, q, red[q * 64 + lane]);
        }
        __syncthreads();
    }
    if (wave != 0) return;
    float* p = partials + (int64_t)blockIdx.x * s.n_net;
    if (lane == 0) p[s.b3] = 0.f;           // (db3 = -sum a needs none of this kernel's work: sphere_reduce_kernel forms it)
    // (lane (j = c, k = h) of the sample products)
#pragma unroll
    for (int mo = 0; mo < 2; ++mo)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = nrn(mo, r, h);
            p[s.w2 + row * 64 + c] = A.w2[mo][0][r];
            p[s.w2 + row * 64 + 32 + c] = A.w2[mo][1][r];
            const int level = 2 * ((c & 15) >> 1) + (c >> 4);
            if (level < gp.n_levels) p[s.w1 + row * s.n_in + 3 + 2 * level + (c & 1)] = A.w1[mo][r];
        }
#pragma unroll
    for (int mo = 0; mo < 2; ++mo) {          // the column sums: the two sample parities, then lane i writes neuron 32 mo + i
        const int row = 32 * mo + c;
#pragma unroll
        for (int a = 0; a < 3; ++a) { float v = A.a[mo][a]; v += __shfl_xor(v, 32); if (h == 0) p[s.w1 + row * s.n_in + a] = v; }
        float v1 = A.b1[mo], v2 = A.b2[mo], v3 = A.w3[mo];
        v1 += __shfl_xor(v1, 32); v2 += __shfl_xor(v2, 32); v3 += __shfl_xor(v3, 32);
        if (h == 0) { p[s.b1 + row] = v1; p[s.b2 + row] = v2; p[s.w3 + row] = v3; }
    }
}

// the fixed-order sum of the workgroups' partials (mlp_reduce_device.hpp).  db3 = -sum a is ONE number, and an fp32 sum of n upstream
// values misses it by ulps of its largest partial sum: the workgroup that owns b3 adds the upstream in double, in a fixed order (thread
// t takes samples t, t + 256, ...; then a tree), so that db3 is right to half an fp32 ulp whatever n
__global__ __launch_bounds__(256) void sphere_reduce_kernel(MlpReduceJob job, const float* __restrict__ draw, int64_t n) {
    __shared__ double part[256];
    mlp_reduce_block(job, blockIdx.x);
    const int b3 = job.n_params - 1;
    if ((int)blockIdx.x != b3 / 16) return;
    double v = 0.0;
    if (draw)
        for (int64_t k = threadIdx.x; k < n; k += 256) v += (double)draw[k];
    part[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) job.dw[b3] = (float)(-part[0]);
}

// what every entry point refuses, in one place
static int check_sphere(const char* who, const perf_grid_desc* grid, int64_t n) {
    PERF_REQUIRE(grid != nullptr, "%s: NULL descriptor", who);
    PERF_REQUIRE(n >= 0, "%s: n < 0", who);
    PERF_REQUIRE(grid->layout == PERF_LAYOUT_TCNN, "%s: tcnn table layout only (layout %d: the line-local layouts are not built)", who, (int)grid->layout);
    PERF_REQUIRE(grid->interpolation == PERF_INTERP_SMOOTHSTEP, "%s: Smoothstep interpolation only (Linear interpolation is not built)", who);
    PERF_REQUIRE(grid->n_levels >= 1 && grid->n_levels <= 16, "%s: 1..16 levels (%d: grids of more than 16 levels are not built)", who, (int)grid->n_levels);
    return PERF_OK;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_sphere_version(void) { return PERF_SPHERE_ABI_VERSION; }

extern "C" int perf_sphere_field_fwd(const perf_grid_desc* grid, const float* table_f32, const float* net_f32, const float* dirs, float* raw,
                                     float* grad_or_null, int64_t n, void* stream) {
    int rc = check_sphere("perf_sphere_field_fwd", grid, n);
    if (rc) return rc;
    GridParams gp;
    rc = fill_params(grid, &gp);
    if (rc) return rc;
    if (n == 0) return PERF_OK;
    PERF_REQUIRE(table_f32 && net_f32 && dirs, "perf_sphere_field_fwd: NULL input pointer");
    PERF_REQUIRE(raw != nullptr, "perf_sphere_field_fwd: NULL output pointer (raw)");
    const int64_t n_tiles = div_up(n, kSphTile);
    const int blocks = (int)(div_up(n_tiles, 4) < 2 * kNumCU ? div_up(n_tiles, 4) : 2 * kNumCU);
    const hipStream_t st = as_stream(stream);
    if (grad_or_null)
        sphere_field_fwd_kernel<true><<<dim3(blocks), dim3(256), kSphFwdLds, st>>>(gp, (const float2*)table_f32, net_f32, dirs, raw, grad_or_null, n);
    else
        sphere_field_fwd_kernel<false><<<dim3(blocks), dim3(256), kSphFwdLds, st>>>(gp, (const float2*)table_f32, net_f32, dirs, raw, nullptr, n);
    PERF_LAUNCH_CHECK("perf_sphere_field_fwd");
    return PERF_OK;
}

extern "C" int64_t perf_sphere_field_bwd_workspace_bytes(const perf_grid_desc* grid, int64_t n) {
    if (check_sphere("perf_sphere_field_bwd_workspace_bytes", grid, n)) return -1;
    return div_up((int64_t)kSphBwdBlocks * sph_net(grid->n_levels).n_net * (int64_t)sizeof(float), 16) * 16;
}

extern "C" int perf_sphere_field_bwd(const perf_grid_desc* grid, const float* table_f32, const float* net_f32, const float* dirs,
                                     const float* draw_or_null, const float* dgrad_or_null, float* grad_out, void* workspace,
                                     int64_t workspace_bytes, int64_t n, void* stream) {
    int rc = check_sphere("perf_sphere_field_bwd", grid, n);
    if (rc) return rc;
    GridParams gp;
    rc = fill_params(grid, &gp);
    if (rc) return rc;
    PERF_REQUIRE(grad_out != nullptr, "perf_sphere_field_bwd: NULL output pointer (grad_out)");
    const SphNet s = sph_net(gp.n_levels);
    const uint64_t entries = gp.offset[gp.n_levels - 1] + gp.size[gp.n_levels - 1];
    const hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(grad_out, 0, ((size_t)s.n_net + 2 * (size_t)entries) * sizeof(float), st) != hipSuccess) {
            set_error("perf_sphere_field_bwd: memset failed");
            return PERF_E_LAUNCH;
        }
        return PERF_OK;
    }
    PERF_REQUIRE(table_f32 && net_f32 && dirs, "perf_sphere_field_bwd: NULL input pointer");
    PERF_REQUIRE(draw_or_null || dgrad_or_null, "perf_sphere_field_bwd: both upstream gradients are NULL (draw, dgrad)");
    PERF_REQUIRE(workspace != nullptr, "perf_sphere_field_bwd: NULL workspace");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "perf_sphere_field_bwd: the workspace must be 16-byte aligned");
    const int64_t need = perf_sphere_field_bwd_workspace_bytes(grid, n);
    PERF_REQUIRE(workspace_bytes >= need, "perf_sphere_field_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    if (hipMemsetAsync(grad_out + s.n_net, 0, 2 * (size_t)entries * sizeof(float), st) != hipSuccess) {
        set_error("perf_sphere_field_bwd: memset failed");
        return PERF_E_LAUNCH;
    }
    // (per call, not once per process: the attribute belongs to the current device's copy of the kernel)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sphere_field_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSphBwdLds) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_sphere_field_bwd: the device does not grant %d bytes of LDS per workgroup", kSphBwdLds);
        return PERF_E_LAUNCH;
    }
    float* partials = (float*)workspace;
    sphere_field_bwd_kernel<<<dim3(kSphBwdBlocks), dim3(256), kSphBwdLds, st>>>(gp, (const float2*)table_f32, net_f32, dirs, draw_or_null, dgrad_or_null,
                                                                                 partials, grad_out + s.n_net, n);
    PERF_LAUNCH_CHECK("perf_sphere_field_bwd");
    const MlpReduceJob job{partials, grad_out, nullptr, nullptr, s.n_net, kSphBwdBlocks, (int32_t)gp.n_levels, (int32_t)div_up(s.n_net, 16) + 1};
    sphere_reduce_kernel<<<dim3((unsigned)job.n_blocks), dim3(256), 0, st>>>(job, draw_or_null, n);
    PERF_LAUNCH_CHECK("perf_sphere_field_bwd(reduce)");
    return PERF_OK;
}
