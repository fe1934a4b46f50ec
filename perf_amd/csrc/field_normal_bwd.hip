// Backward of (sigma, grad_x sigma) with respect to the density field's parameters (perf_field_grad_x_bwd): what a loss on surface
// normals needs during training.  One kernel; a wave owns a tile of 32 samples as in field_grad_x_kernel, whose steps 1-3 it runs
// unchanged (field_normal_device.hpp): F (packed features), J = dF/dx01 (dF[r][a]), the masks (hb), y (o[0]), p = W1^T (m . w_o) (dx).
//
// Per sample, with the upstream dsigma (scalar) and dg (world units), e = 1 / (hi - lo):
//     u = dg . e . sel,   Fd = J u  (in-lane),   yd = p . Fd  (in-lane + one cross-half add),   so that dg . g = a'(y) yd
//     c_y = sel dsigma a'(y) + a''(y) yd,   c_t = a'(y)
//     (Exponential: a'' = a' where y - shift < 15, else 0 -- the truncated exponential differentiated once more;
//      Sigmoid: a'' = s (1 - s) (1 - 2 s);  None: a'' = 0)
// and the whole parameter gradient is p, m . w_o, F, Fd, H, Hd times those two scalars, which stay in fp32 to the end -- the result is
// linear in (dsigma, dg) to fp32 rounding, and nothing of it can leave the range of a 16-bit type:
//     dWo[0, j]  = sum c_y H_j + c_t Hd_j,  Hd = m . (W1 Fd)  -- one more forward chain on the packed Fd (scaled per sample by the power
//                  of two that brings its largest element to [1, 2): exact, undone in c_t), masked, added IN-LANE in fp32 (32 registers
//                  in the D layout); the 32 lanes of a half are added once per block
//     dW1[j, k]  = sum (m . w_o)_j G_k,  G = c_y F + c_t Fd (fp32)  -- mlp_bwd_kernel's weight-gradient products (LDS transpose, 32x32x16
//                  MFMA), with G cut into THREE bf16 pieces (8 + 8 + 8 bits: G to the last bit) that take the tile one after the other;
//                  the products run on the bf16 MFMA for both weight types -- an fp16 weight is the exact sum of two bf16 numbers, so
//                  its A tile comes in two pieces -- because c_y F of a trunc_exp density does not fit fp16
//     dtable[idx_c(l), f] += p_{l,f} (c_y w_c + c_t W'_c),  W'_c = sum_a u_a dw_c/dx01_a
// ReLU has no second derivative; positions are not trained.  The other 15 padded rows of Wo get exactly 0.
//
// Network part: accumulators per wave across tiles, one partial per workgroup, summed by mlp_reduce_kernel in a fixed order --
// deterministic, and independent of how many samples of the capacity n are live (n_dev).
// Table part: the lane that formed a level's features recomputes the corner indices and weights (64 indices per lane do not fit
// beside the accumulators) and scatters straight into the zero-filled table part with fp32 global atomics -- flat ~2e10 / s on gfx950
// (hashgrid_bwd_atomic_kernel): 32 k kept samples x 16 levels x 16 atomics = 8.4 M: 0.6 ms measured, 1.4e10 / s.  This consumer's batches are the kept
// samples of a step (10^4..10^5); no feature gradient goes through memory.  The table part therefore depends, in its last bits, on
// the order the atomics retire in.  Plain vector stores and vector atomics only.
//
// Registers: 48 (J) + 16 (Fd, then G) + 16 (p) + 16 + 16 (masks, pulled-back operand) + 32 + 32 accumulators; J dies before the MFMA
// temporaries of steps 5-6 are live.  The compiler's report (registers, scratch) and the workgroups per CU it allows are recorded in
// DESIGN.md 5.5; LDS: 16 KB of fragments + 2 (bf16) or 3 (fp16) wave-private tiles of 4.5 KB per wave.
//
// Built: tcnn table layout, Linear interpolation, one hidden layer, up to 16 levels, bf16 / fp16.  Everything else is refused.
#include "field_normal_device.hpp"
#include "mlp_reduce_device.hpp"
#include "../../include/perf_hip_ext.h"

namespace perf {

struct GradXBwdIn {
    GridParams gp;
    const uint32_t* table;
    const float* x01;
    const float* dsigma;        // [n] or NULL
    const float* dgrad;         // [n, 3] or NULL
    float inv_extent[3];
};

constexpr int kGradXBwdPerCU = 2;

template <typename T16>
struct GradXBwdTiles {
    static constexpr int pieces_a = std::is_same<T16, FP16>::value ? 2 : 1;        // bf16 pieces of a weight
    static constexpr int per_wave = pieces_a + 1;
    template <int KS>
    static constexpr int lds_bytes() { return GradXFrags<KS>::n * 1024 + 4 * per_wave * kTile * kPitchT * 2; }
};

template <typename T16, int KS>
__global__ __launch_bounds__(256, kGradXBwdPerCU) void field_grad_x_bwd_kernel(MlpParams mp, const uint16_t* __restrict__ w,
                                                                               const uint8_t* __restrict__ sel, float* __restrict__ partials,
                                                                               float* __restrict__ gtable, int64_t n,
                                                                               const int64_t* __restrict__ n_dev, GradXBwdIn in) {
    using L = Layout<1, KS>;
    constexpr int kFrag = GradXFrags<KS>::n;
    const int64_t n_live = live_count(n, n_dev);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* frag = reinterpret_cast<u32x4*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    constexpr int kPiecesA = GradXBwdTiles<T16>::pieces_a;
    // (mlp_bwd_kernel's wave-private tiles: the A tile(s) [sample][neuron position], then the B tile [sample][input position])
    uint16_t* tA = reinterpret_cast<uint16_t*>(smem + kFrag * 1024) + wave * (GradXBwdTiles<T16>::per_wave * kTile * kPitchT);
    uint16_t* tB = tA + kPiecesA * kTile * kPitchT;
    const int off32 = tr_offset32(lane);
    stage_grad_x_fragments<KS>(w, frag);
    __syncthreads();
    f32x16 gW1[2], gWo[2];          // gWo[m][r]: this lane's samples' part of dWo[0][32 m + d_row(r, h)]
#pragma unroll
    for (int m = 0; m < 2; ++m) { gW1[m] = f32x16{0}; gWo[m] = f32x16{0}; }
    const int64_t n_tiles = (n_live + kTile - 1) / kTile;
    const int64_t tile_step = (int64_t)gridDim.x * 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += tile_step) {
        const int64_t si = tile * kTile + c;
        // a sample outside the box (or past the end) contributes nothing: it is not gathered either
        const bool live = si < n_live && (sel ? sel[si] != 0 : true);
        float x = 0.5f, y = 0.5f, z = 0.5f, ds = 0.f, u[3] = {0.f, 0.f, 0.f};
        if (live) {
            x = in.x01[3 * si]; y = in.x01[3 * si + 1]; z = in.x01[3 * si + 2];
            if (in.dsigma) ds = in.dsigma[si];
            if (in.dgrad) {
#pragma unroll
                for (int a = 0; a < 3; ++a) u[a] = in.dgrad[3 * si + a] * in.inv_extent[a];
            }
        }
        // ---- 1.-3. (field_normal_device.hpp)
        u32x4 b1[KS], hb[4], dh[4];
        float dF[8 * KS][3];
        features_and_derivatives<T16, KS>(in.gp, in.table, mp.n_levels, live, h, x, y, z, b1, dF);
        f32x16 o, dx;
        forward_and_pull_back<T16, KS>(frag, lane, b1, hb, dh, o, dx);
        // ---- the A tile(s) of the dW1 products go to LDS now: the pulled-back operand is not needed in registers after this
        __builtin_amdgcn_wave_barrier();
        if constexpr (kPiecesA == 1) {
            lds_put_hidden(tA, dh, c, h);
        } else {                                    // fp16 weight = bf16 piece + bf16 piece, exactly
#pragma unroll
            for (int s = 0; s < 4; ++s) {           // (k-step by k-step: eight temporaries, not thirty-two)
                u32x4 hi16, lo16;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = T16::lo(dh[s][i]), b = T16::hi(dh[s][i]);
                    hi16[i] = BF16::pack(a, b);
                    lo16[i] = BF16::pack(a - BF16::lo(hi16[i]), b - BF16::hi(hi16[i]));
                }
                *reinterpret_cast<u32x4*>(tA + c * kPitchT + 16 * s + 8 * h) = hi16;          // (lds_put_hidden's slot)
                *reinterpret_cast<u32x4*>(tA + kTile * kPitchT + c * kPitchT + 16 * s + 8 * h) = lo16;
            }
        }
        // ---- 4. Fd = J u, yd = p . Fd
        float Fd[8 * KS], yd = 0.f;
#pragma unroll
        for (int r = 0; r < 8 * KS; ++r) {
            Fd[r] = fmaf(dF[r][2], u[2], fmaf(dF[r][1], u[1], dF[r][0] * u[0]));
            yd = fmaf(dx[r], Fd[r], yd);
        }
        yd += __shfl_xor(yd, 32);
        const float yv = __shfl(o[0], c);           // (row 0 of the output is register 0 of half 0)
        float d1, d2;
        if (mp.out_act == PERF_ACT_SIGMOID) { const float s_ = 1.0f / (1.0f + expf(-yv)); d1 = s_ * (1.0f - s_); d2 = d1 * (1.0f - 2.0f * s_); }
        else if (mp.out_act == PERF_ACT_EXP) { d1 = expf(fminf(yv - mp.exp_shift, 15.0f)); d2 = yv - mp.exp_shift < 15.0f ? d1 : 0.f; }
        else { d1 = 1.0f; d2 = 0.f; }
        const float c_y = live ? fmaf(d2, yd, ds * d1) : 0.f;
        const float c_t = live ? d1 : 0.f;
        // ---- 5. dWo[0][:] += c_y H + c_t m . (W1 Fd): the chain runs on Fd scaled by a power of two (exact), c_t carries it back
        float mx = 0.f;
#pragma unroll
        for (int r = 0; r < 8 * KS; ++r) mx = fmaxf(mx, fabsf(Fd[r]));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const uint32_t eb = (__float_as_uint(mx) >> 23) & 0xffu;           // (biased exponent of the sample's largest |Fd|)
        const bool scaled = eb >= 2u && eb <= 252u;
        const float down = scaled ? __uint_as_float((254u - eb) << 23) : 1.0f, up = scaled ? __uint_as_float(eb << 23) : 1.0f;
        const float c_tu = c_t * up;
        u32x4 fb[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) fb[s][i] = T16::pack(Fd[2 * (4 * s + i)] * down, Fd[2 * (4 * s + i) + 1] * down);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            f32x16 acc = f32x16{0};
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = T16::mfma(frag[(L::f_a1 + m * KS + s) * 64 + lane], fb[s], acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {          // register 8 t + 2 i + e of block m <-> half e of hb[2 m + t][i] (relu_pack_plain)
                const uint32_t word = hb[2 * m + (r >> 3)][(r & 7) >> 1];
                const float hv = (r & 1) ? T16::hi(word) : T16::lo(word);
                gWo[m][r] += hv != 0.f ? fmaf(c_tu, acc[r], c_y * hv) : 0.f;
            }
        }
        // ---- 6. dW1[64 x n_in_pad] += (m . w_o) G^T (mlp_bwd_kernel's products, one block of 32 input features), G = c_y F + c_t Fd
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = 2 * (4 * s + i);
                Fd[q] = fmaf(c_t, Fd[q], c_y * T16::lo(b1[s][i]));
                Fd[q + 1] = fmaf(c_t, Fd[q + 1], c_y * T16::hi(b1[s][i]));
            }
#pragma unroll
        for (int piece = 0; piece < 3; ++piece) {
            u32x4 gb[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q = 2 * (4 * s + i);
                    gb[s][i] = BF16::pack(Fd[q], Fd[q + 1]);
                    Fd[q] -= BF16::lo(gb[s][i]); Fd[q + 1] -= BF16::hi(gb[s][i]);          // (the remainder of a rounding is exact)
                }
            __builtin_amdgcn_wave_barrier();        // (the products of the piece before have read the tile)
#pragma unroll
            for (int s = 0; s < KS; ++s)            // position 16 s + 8 h + j holds input feature 2 (8 s + 2 (j >> 1) + h) + (j & 1)
                *reinterpret_cast<u32x4*>(tB + c * kPitchT + 16 * s + 8 * h) = gb[s];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                u32x4 b = lds_get_frag(tB, off32, 0, s);             // (every lane takes part in the transposing read)
                if (c >= L::n_in_pad) b = u32x4{0, 0, 0, 0};
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int pa = 0; pa < kPiecesA; ++pa)
                        gW1[m] = BF16::mfma(lds_get_frag(tA + pa * kTile * kPitchT, off32, m, s), b, gW1[m]);
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 7. the table part: d table[idx_c] += p (c_y w_c + c_t W'_c), straight into global memory
        if (live) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int level = 8 * s + 2 * i + h;
                    const int q = 2 * (4 * s + i);
                    const float p0 = dx[q], p1 = dx[q + 1];
                    if (level >= mp.n_levels || (p0 == 0.f && p1 == 0.f)) continue;
                    const float scale = in.gp.scale[level];
                    const uint32_t size = in.gp.size[level];
                    const Corners cr = corners_of(x, y, z, scale, in.gp.res[level], size, in.gp.hashed[level] != 0);
                    const float fx = cr.f[0], fy = cr.f[1], fz = cr.f[2];
                    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
                    const float ux = u[0] * scale, uy = u[1] * scale, uz = u[2] * scale;
                    float* t = gtable + 2 * in.gp.offset[level];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
                        const float wc = (wx[bx] * wy[by]) * wz[bz];
                        const float wyz = wy[by] * wz[bz], wxz = wx[bx] * wz[bz], wxy = wx[bx] * wy[by];
                        const float dwc = fmaf(bz ? uz : -uz, wxy, fmaf(by ? uy : -uy, wxz, (bx ? ux : -ux) * wyz));
                        const float coef = fmaf(c_t, dwc, c_y * wc);
                        const uint32_t idx = cr.idx[k];
                        if (idx < size && coef != 0.f) {            // (corners_of keeps a live sample's indices inside the level)
                            unsafeAtomicAdd(t + 2 * (uint64_t)idx, coef * p0);
                            unsafeAtomicAdd(t + 2 * (uint64_t)idx + 1, coef * p1);
                        }
                    }
                }
        }
    }
    // ---- block reduction of the four waves' accumulators through LDS (lane-linear slots), then ONE partial per block -> global
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    static_assert(4 * 16 * 64 * 4 <= GradXBwdTiles<T16>::template lds_bytes<KS>(), "reduction scratch exceeds LDS");
    for (int src = 1; src < 4; ++src) {
        if (wave == src) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) { red[(m * 16 + r) * 64 + lane] = gW1[m][r]; red[((2 + m) * 16 + r) * 64 + lane] = gWo[m][r]; }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) { gW1[m][r] += red[(m * 16 + r) * 64 + lane]; gWo[m][r] += red[((2 + m) * 16 + r) * 64 + lane]; }
        }
        __syncthreads();
    }
    if (wave != 0) return;
    float* p = partials + (int64_t)blockIdx.x * L::n_params;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {       // rows and columns of the products are channel POSITIONS of the tiles (mlp_bwd_kernel)
            const int row = position_neuron(32 * m + d_row(r, h));
            const int in_f = (c & ~15) + 4 * ((c & 7) >> 1) + 2 * ((c >> 3) & 1) + (c & 1);
            if (c < L::n_in_pad) p[L::w1_off + row * L::n_in_pad + in_f] = gW1[m][r];
        }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {       // the 32 samples of a half, in a fixed order
            float v = gWo[m][r];
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (c == 0) p[L::wo_off + 32 * m + d_row(r, h)] = v;
        }
    for (int k = lane; k < 15 * 64; k += 64) p[L::wo_off + 64 + k] = 0.f;
}

template <typename T16, int KS>
static void launch_grad_x_bwd(int blocks, hipStream_t st, MlpParams mp, const uint16_t* w, const uint8_t* sel, float* partials, float* gtable,
                              int64_t n, const int64_t* n_dev, const GradXBwdIn& in) {
    constexpr int lds_bytes = GradXBwdTiles<T16>::template lds_bytes<KS>();
    static std::once_flag attr_once;            // (one flag per template instance)
    std::call_once(attr_once, []() {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&field_grad_x_bwd_kernel<T16, KS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    });
    field_grad_x_bwd_kernel<T16, KS><<<dim3(blocks), dim3(256), lds_bytes, st>>>(mp, w, sel, partials, gtable, n, n_dev, in);
}

// what both entry points refuse, in one place; ks out
static int check_grad_x_bwd(const perf_grid_desc* grid, const perf_mlp_desc* mlp, int64_t n, int* ks) {
    PERF_REQUIRE(grid && mlp, "perf_field_grad_x_bwd: NULL descriptor");
    PERF_REQUIRE(n >= 0, "perf_field_grad_x_bwd: n < 0");
    PERF_REQUIRE(mlp->n_levels == grid->n_levels, "perf_field_grad_x_bwd: the MLP takes %d levels, the grid has %d", (int)mlp->n_levels, (int)grid->n_levels);
    PERF_REQUIRE(grid->layout == PERF_LAYOUT_TCNN, "perf_field_grad_x_bwd: tcnn table layout only (layout %d: the line-local layouts have no input gradient)", (int)grid->layout);
    PERF_REQUIRE(grid->interpolation == PERF_INTERP_LINEAR, "perf_field_grad_x_bwd: Linear interpolation only (Smoothstep is not built)");
    PERF_REQUIRE(grid->n_levels >= 1 && grid->n_levels <= 16, "perf_field_grad_x_bwd: 1..16 levels (%d: grids of more than 16 levels are not built)", (int)grid->n_levels);
    int nh;
    int rc = check_mlp(mlp, &nh, ks);
    if (rc) return rc;
    PERF_REQUIRE(nh == 1, "perf_field_grad_x_bwd: one hidden layer only (the density network); n_hidden_layers %d is not built", nh);
    return PERF_OK;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_ext_version(void) { return PERF_EXT_ABI_VERSION; }

extern "C" int64_t perf_field_grad_x_bwd_workspace_bytes(const perf_grid_desc* grid, const perf_mlp_desc* mlp, int64_t n) {
    int ks;
    if (check_grad_x_bwd(grid, mlp, n, &ks)) return -1;
    const int blocks = mlp_blocks(n > 0 ? n : 1, kGradXBwdPerCU);
    return (int64_t)blocks * n_params_rt(1, ks) * (int64_t)sizeof(float);
}

extern "C" int perf_field_grad_x_bwd(const perf_grid_desc* grid, const perf_mlp_desc* mlp, const float* x01, const uint8_t* sel,
                                     const void* table16, const void* w16, const float* inv_extent, const float* dsigma, const float* dgrad,
                                     float* grad, void* workspace, int64_t workspace_bytes, int64_t n, const int64_t* n_dev, int dtype,
                                     void* stream) {
    int ks;
    int rc = check_grad_x_bwd(grid, mlp, n, &ks);
    if (rc) return rc;
    PERF_REQUIRE(dtype == PERF_DTYPE_BF16 || dtype == PERF_DTYPE_FP16, "perf_field_grad_x_bwd: bad dtype %d", dtype);
    GradXBwdIn in;
    rc = fill_params(grid, &in.gp);
    if (rc) return rc;
    PERF_REQUIRE(grad != nullptr, "perf_field_grad_x_bwd: NULL output pointer (grad)");
    const int n_net = n_params_rt(1, ks);
    const uint64_t entries = in.gp.offset[in.gp.n_levels - 1] + in.gp.size[in.gp.n_levels - 1];
    const hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(grad, 0, ((size_t)n_net + 2 * (size_t)entries) * sizeof(float), st) != hipSuccess) {
            set_error("perf_field_grad_x_bwd: memset failed");
            return PERF_E_LAUNCH;
        }
        return PERF_OK;
    }
    PERF_REQUIRE(x01 && table16 && w16, "perf_field_grad_x_bwd: NULL input pointer");
    PERF_REQUIRE(dsigma || dgrad, "perf_field_grad_x_bwd: both upstream gradients are NULL (dsigma, dgrad)");
    PERF_REQUIRE(workspace != nullptr, "perf_field_grad_x_bwd: NULL workspace");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "perf_field_grad_x_bwd: the workspace must be 16-byte aligned");
    const int64_t need = perf_field_grad_x_bwd_workspace_bytes(grid, mlp, n);
    PERF_REQUIRE(workspace_bytes >= need, "perf_field_grad_x_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    in.table = (const uint32_t*)table16; in.x01 = x01; in.dsigma = dsigma; in.dgrad = dgrad;
    for (int a = 0; a < 3; ++a) in.inv_extent[a] = inv_extent ? inv_extent[a] : 1.0f;
    if (hipMemsetAsync(grad + n_net, 0, 2 * (size_t)entries * sizeof(float), st) != hipSuccess) {
        set_error("perf_field_grad_x_bwd: memset failed");
        return PERF_E_LAUNCH;
    }
    MlpParams mp{mlp->n_levels, mlp->n_out, mlp->out_act, mlp->exp_shift};
    const int blocks = mlp_blocks(n, kGradXBwdPerCU);
    float* partials = (float*)workspace;
    if (dtype == PERF_DTYPE_BF16) {
        if (ks == 1) launch_grad_x_bwd<BF16, 1>(blocks, st, mp, (const uint16_t*)w16, sel, partials, grad + n_net, n, n_dev, in);
        else launch_grad_x_bwd<BF16, 2>(blocks, st, mp, (const uint16_t*)w16, sel, partials, grad + n_net, n, n_dev, in);
    } else {
        if (ks == 1) launch_grad_x_bwd<FP16, 1>(blocks, st, mp, (const uint16_t*)w16, sel, partials, grad + n_net, n, n_dev, in);
        else launch_grad_x_bwd<FP16, 2>(blocks, st, mp, (const uint16_t*)w16, sel, partials, grad + n_net, n, n_dev, in);
    }
    PERF_LAUNCH_CHECK("perf_field_grad_x_bwd");
    const MlpReduceJob job{partials, grad, nullptr, nullptr, n_net, blocks, (int32_t)mlp->n_levels, (int32_t)div_up(n_net, 16) + 1};
    perf_internal_launch_mlp_reduce(job, stream);
    PERF_LAUNCH_CHECK("perf_field_grad_x_bwd(reduce)");
    return PERF_OK;
}
