// The alignment step of the joint geometry predictor (include/perf_hip_joint.h): sampling, losses and gradients around the fused sphere
// distance field.  Three entry points, five kernels:
//   joint_sample_kernel        one thread per sample: eleven bilinear channel reads of the three view maps, the panorama look-up
//   joint_loss_kernel          one thread per sample: the four per-sample loss terms, d/dd, d/dg, the per-sample part of d/dscale,
//                              the bilinear scatter of d/ddb and d/dnb (fp32 global atomics, 'hybrid' phase only); one partial per
//                              workgroup
//   joint_loss_finish_kernel   one workgroup: the partials in a fixed order, L_reg, d/dscale per view, the total
//   joint_tv_kernel            streaming: a thread owns 8 rows x 4 columns of one image, issues the ten float4 row loads and sixteen
//                              neighbour loads of its strip before the first use, writes the gradient as float4s; one partial per workgroup
//   joint_tv_finish_kernel     one workgroup: the partials in a fixed order
// A sample's arithmetic is carried in double between fp32 loads and fp32 stores: N = 15,360 threads on 256 CUs wait for memory and for
// launches, not for the vector unit, and the double rate of gfx950 is half the fp32 rate.  Every sum over samples is a tree in LDS over
// a workgroup and then a fixed-order sum of the workgroups' partials: two runs give identical bits.  Plain vector loads and stores and
// vector atomics only.
#include "common.hpp"
#include "../../include/perf_hip_joint.h"

namespace perf {

constexpr int kJtBlock = 256;
constexpr int kJtRec = PERF_JOINT_RECORD;
constexpr int kTvRows = 8;                  // rows of a thread's strip
constexpr int kTvMaxBlocks = 4096;          // workgroups of the streaming kernel at most == partials of the TV value
constexpr double kPi = 3.14159265358979323846;

// torch's grid_sample position on an axis of S texels, border padding: the two corners and their weights
struct Axis { int i0, i1; double w0, w1; };

__device__ __forceinline__ Axis axis_of(double c, int S) {
    double f = ((c + 1.0) * (double)S - 1.0) * 0.5;
    f = fmin(fmax(f, 0.0), (double)(S - 1));
    const double fl = floor(f);
    Axis a;
    a.i0 = (int)fl;
    a.i1 = a.i0 + 1;
    a.w1 = f - fl;
    a.w0 = (fl + 1.0) - f;
    return a;
}

// one channel [S_y, S_x]; a corner outside the map has weight 0 and is not read
__device__ __forceinline__ double bilinear(const float* __restrict__ img, const Axis& ax, const Axis& ay, int Sx, int Sy) {
    const bool in_x = ax.i1 < Sx, in_y = ay.i1 < Sy;
    const float* r0 = img + (int64_t)ay.i0 * Sx;
    const float* r1 = img + (int64_t)(in_y ? ay.i1 : ay.i0) * Sx;
    const int x1 = in_x ? ax.i1 : ax.i0;
    const double nw = r0[ax.i0], ne = in_x ? (double)r0[x1] : 0.0, sw = in_y ? (double)r1[ax.i0] : 0.0, se = (in_x && in_y) ? (double)r1[x1] : 0.0;
    return ((nw * (ax.w0 * ay.w0) + ne * (ax.w1 * ay.w0)) + sw * (ax.w0 * ay.w1)) + se * (ax.w1 * ay.w1);
}

__device__ __forceinline__ void scatter(float* __restrict__ img, const Axis& ax, const Axis& ay, int Sx, int Sy, double v) {
    const bool in_x = ax.i1 < Sx, in_y = ay.i1 < Sy;
    float* r0 = img + (int64_t)ay.i0 * Sx;
    unsafeAtomicAdd(r0 + ax.i0, (float)(v * (ax.w0 * ay.w0)));
    if (in_x) unsafeAtomicAdd(r0 + ax.i1, (float)(v * (ax.w1 * ay.w0)));
    if (in_y) {
        float* r1 = img + (int64_t)ay.i1 * Sx;
        unsafeAtomicAdd(r1 + ax.i0, (float)(v * (ax.w0 * ay.w1)));
        if (in_x) unsafeAtomicAdd(r1 + ax.i1, (float)(v * (ax.w1 * ay.w1)));
    }
}

// smooth-L1 and its derivative
__device__ __forceinline__ double sl1(double x, double beta) {
    const double a = fabs(x);
    return a < beta ? 0.5 * x * x / beta : a - 0.5 * beta;
}
__device__ __forceinline__ double sl1_d(double x, double beta) {
    return fabs(x) < beta ? x / beta : (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0));
}
// torch's softplus (beta = 1, threshold = 20) and its derivative
__device__ __forceinline__ double softplus1(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double sigmoid1(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

// the sum of one value per thread over the workgroup, in a fixed order (a tree in LDS); every thread gets it
__device__ __forceinline__ double block_sum(double v, double* part) {
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
    for (int w = kJtBlock / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(kJtBlock) void joint_sample_kernel(const float* __restrict__ sup, const float* __restrict__ bias_d,
                                                                const float* __restrict__ bias_n, const float* __restrict__ ref,
                                                                const float* __restrict__ coords, const float* __restrict__ u_given, int64_t N, int64_t B,
                                                                int R, int Rn, int H, int W, float* __restrict__ u_out, float* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * kJtBlock + threadIdx.x;
    if (i >= N) return;
    const int64_t p = i / B;
    const double cx = coords[2 * i], cy = coords[2 * i + 1];
    const Axis ax = axis_of(cx, R), ay = axis_of(cy, R);
    const int64_t plane = (int64_t)R * R;
    const float* s = sup + p * 7 * plane;
    double v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = bilinear(s + c * plane, ax, ay, R, R);
    const double db = bilinear(bias_d + p * plane, ax, ay, R, R);
    const Axis bx = axis_of(cx, Rn), by = axis_of(cy, Rn);
    const int64_t nplane = (int64_t)Rn * Rn;
    double nb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nb[c] = bilinear(bias_n + (p * 3 + c) * nplane, bx, by, Rn, Rn);
    double ux, uy, uz;
    if (u_given) {          // the caller's directions, bit for bit
        ux = u_given[3 * i]; uy = u_given[3 * i + 1]; uz = u_given[3 * i + 2];
    } else {
        const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        ux = v[0] / len; uy = v[1] / len; uz = v[2] / len;
        u_out[3 * i] = (float)ux; u_out[3 * i + 1] = (float)uy; u_out[3 * i + 2] = (float)uz;
    }
    // the panorama look-up
    const double beta = asin(uz), alpha = atan2(uy, ux);
    const double row = -beta / kPi + 0.5, col = -(alpha / (2.0 * kPi)) + 0.5;
    const Axis px = axis_of(col * 2.0 - 1.0, W), py = axis_of(row * 2.0 - 1.0, H);
    const double pr = bilinear(ref, px, py, W, H), pm = bilinear(ref + (int64_t)H * W, px, py, W, H);
    f32x4* r = reinterpret_cast<f32x4*>(rec + kJtRec * i);
    f32x4 q0, q1, q2;
    q0[0] = (float)v[3]; q0[1] = (float)db; q0[2] = (float)v[4]; q0[3] = (float)v[5];
    q1[0] = (float)v[6]; q1[1] = (float)nb[0]; q1[2] = (float)nb[1]; q1[3] = (float)nb[2];
    q2[0] = (float)pr; q2[1] = (float)pm; q2[2] = 0.f; q2[3] = 0.f;
    r[0] = q0; r[1] = q1; r[2] = q2;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void unit3(double* a) {
    const double l = sqrt(dot3(a, a));
    a[0] /= l; a[1] /= l; a[2] /= l;
}

struct JointLossArgs {
    const float *rec, *coords, *scale, *u, *d, *g, *o, *tv;
    float *losses, *dd, *dg, *dscale, *gbias_d, *gbias_n;
    double* partials;       // [n_blocks][4]: sums of the L_d, L_n and L_ref elements
    double* contrib;        // [N]: a sample's part of d total / d scale_p
    int64_t N, B;
    int P, R, Rn, n_blocks;
    double w_ref, w_reg, w_n, w_ntv;
};

__global__ __launch_bounds__(kJtBlock) void joint_loss_kernel(JointLossArgs A) {
    __shared__ double part[kJtBlock];
    const int64_t i = (int64_t)blockIdx.x * kJtBlock + threadIdx.x;
    double e_d = 0.0, e_n = 0.0, e_ref = 0.0;
    if (i < A.N) {
        const int64_t p = i / A.B;
        const double inv_n = 1.0 / (double)A.N;
        const f32x4* r = reinterpret_cast<const f32x4*>(A.rec + kJtRec * i);
        const f32x4 q0 = r[0], q1 = r[1], q2 = r[2];
        const double sd = q0[0], db = q0[1], pr = q2[0], pm = q2[1];
        double rn[3] = {(double)q0[2] + (double)q1[1], (double)q0[3] + (double)q1[2], (double)q1[0] + (double)q1[3]};
        const double rn_len = sqrt(dot3(rn, rn));
        rn[0] /= rn_len; rn[1] /= rn_len; rn[2] /= rn_len;
        const double sc = A.scale[p];
        const double d = A.d[i];
        const double u[3] = {A.u[3 * i], A.u[3 * i + 1], A.u[3 * i + 2]};
        const double g[3] = {A.g[3 * i], A.g[3 * i + 1], A.g[3 * i + 2]};
        const double o[3] = {A.o[3 * i], A.o[3 * i + 1], A.o[3 * i + 2]};
        // the distance term
        const double x_d = (sd * softplus1(sc) + db) - d;
        e_d = sl1(x_d, 0.5);
        const double d_rd = sl1_d(x_d, 0.5) * inv_n;            // d total / d rd == d total / d db
        A.contrib[i] = d_rd * sd * sigmoid1(sc);
        // the panorama term
        const double live = pm < 0.5 ? 1.0 : 0.0, x_r = pr - d;
        e_ref = sl1(x_r, 0.01) * live;
        A.dd[i] = (float)(-d_rd - A.w_ref * sl1_d(x_r, 0.01) * live * inv_n);
        // the normal term: tangents b = unit(u x o), a = unit(b x u)
        double t[2][3];
        cross3(u, o, t[1]); unit3(t[1]);
        cross3(t[1], u, t[0]); unit3(t[0]);
        double dgs[3] = {0.0, 0.0, 0.0}, drn[3] = {0.0, 0.0, 0.0};
        const double k_n = A.w_n * 0.5 * inv_n;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double q = dot3(g, t[k]);
            double w[3] = {q * u[0] + t[k][0], q * u[1] + t[k][1], q * u[2] + t[k][2]};
            const double wl = sqrt(dot3(w, w));
            const double v[3] = {w[0] / wl, w[1] / wl, w[2] / wl};
            const double e = dot3(v, rn);
            e_n += sl1(e, 0.5);
            const double de = k_n * sl1_d(e, 0.5);
            // dv = de rn;  dw = (dv - v (v . dv)) / |w|;  dq = dw . u;  dg += dq t
            const double vd = de * e;
            const double dw[3] = {(de * rn[0] - v[0] * vd) / wl, (de * rn[1] - v[1] * vd) / wl, (de * rn[2] - v[2] * vd) / wl};
            const double dq = dot3(dw, u);
#pragma unroll
            for (int c = 0; c < 3; ++c) { dgs[c] += dq * t[k][c]; drn[c] += de * v[c]; }
        }
        A.dg[3 * i] = (float)dgs[0]; A.dg[3 * i + 1] = (float)dgs[1]; A.dg[3 * i + 2] = (float)dgs[2];
        if (A.gbias_d) {        // the 'hybrid' phase: the two maps are trained
            const double cx = A.coords[2 * i], cy = A.coords[2 * i + 1];
            const Axis ax = axis_of(cx, A.R), ay = axis_of(cy, A.R);
            scatter(A.gbias_d + p * (int64_t)A.R * A.R, ax, ay, A.R, A.R, d_rd);
            const double rd_ = dot3(rn, drn);
            const Axis bx = axis_of(cx, A.Rn), by = axis_of(cy, A.Rn);
            const int64_t nplane = (int64_t)A.Rn * A.Rn;
#pragma unroll
            for (int c = 0; c < 3; ++c) scatter(A.gbias_n + (p * 3 + c) * nplane, bx, by, A.Rn, A.Rn, (drn[c] - rn[c] * rd_) / rn_len);
        }
    }
    const double s_d = block_sum(e_d, part), s_n = block_sum(e_n, part), s_r = block_sum(e_ref, part);
    if (threadIdx.x == 0) {
        double* out = A.partials + 4 * (int64_t)blockIdx.x;
        out[0] = s_d; out[1] = s_n; out[2] = s_r; out[3] = 0.0;
    }
}

__global__ __launch_bounds__(kJtBlock) void joint_loss_finish_kernel(JointLossArgs A) {
    __shared__ double part[kJtBlock];
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < A.n_blocks; b += kJtBlock)
        for (int k = 0; k < 3; ++k) s[k] += A.partials[4 * (int64_t)b + k];
    double sp = 0.0;
    for (int p = threadIdx.x; p < A.P; p += kJtBlock) sp += softplus1((double)A.scale[p]);
    const double t_d = block_sum(s[0], part), t_n = block_sum(s[1], part), t_r = block_sum(s[2], part);
    const double mean_sp = block_sum(sp, part) / (double)A.P;
    const double l_reg = (mean_sp - 1.0) * (mean_sp - 1.0);
    // d total / d scale_p: the view's samples in their order, then the L_reg term
    for (int p = threadIdx.x; p < A.P; p += kJtBlock) {
        const double* c = A.contrib + (int64_t)p * A.B;
        double acc = 0.0;
#pragma unroll 8
        for (int64_t b = 0; b < A.B; ++b) acc += c[b];
        A.dscale[p] = (float)(acc + A.w_reg * 2.0 * (mean_sp - 1.0) * sigmoid1((double)A.scale[p]) / (double)A.P);
    }
    if (threadIdx.x == 0) {
        const double l_d = t_d / (double)A.N, l_n = t_n / (2.0 * (double)A.N), l_ref = t_r / (double)A.N;
        const double tv_d = A.tv ? (double)A.tv[0] : 0.0, tv_n = A.tv ? (double)A.tv[1] : 0.0;
        A.losses[0] = (float)l_d; A.losses[1] = (float)l_n; A.losses[2] = (float)l_reg; A.losses[3] = (float)l_ref;
        A.losses[4] = (float)tv_d; A.losses[5] = (float)tv_n;
        A.losses[6] = (float)(((((A.w_ref * l_ref + l_d) + A.w_reg * l_reg) + A.w_n * l_n) + tv_d) + A.w_ntv * tv_n);
        A.losses[7] = 0.f;
    }
}

// ---- total variation ---------------------------------------------------------------------------------------------------------------
struct TvRow { float v[4]; };

template <bool kVec>
__device__ __forceinline__ TvRow tv_row(const float* __restrict__ row, int c0, int W) {
    TvRow r;
    if (kVec) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(row + c0);
        r.v[0] = q[0]; r.v[1] = q[1]; r.v[2] = q[2]; r.v[3] = q[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = row[c0 + k < W ? c0 + k : W - 1];          // (clamped: a column past the map is never used)
    }
    return r;
}

template <bool kVec>
__global__ __launch_bounds__(kJtBlock) void joint_tv_kernel(const float* __restrict__ map, float* __restrict__ grad, int64_t n_img, int H, int W,
                                                            double weight, double inv_nv, double inv_nh, double* __restrict__ partials) {
    __shared__ double part[kJtBlock];
    constexpr double kBeta = 0.01;
    const int ncg = (W + 3) / 4, nrc = (H + kTvRows - 1) / kTvRows;
    const int64_t total = n_img * nrc * ncg;
    double sv = 0.0, sh = 0.0;
    for (int64_t item = (int64_t)blockIdx.x * kJtBlock + threadIdx.x; item < total; item += (int64_t)gridDim.x * kJtBlock) {
        const int cg = (int)(item % ncg);
        const int64_t t = item / ncg;
        const int rc = (int)(t % nrc);
        const int64_t img = t / nrc;
        const int c0 = cg * 4, r0 = rc * kTvRows, r1 = r0 + kTvRows < H ? r0 + kTvRows : H;
        const float* base = map + img * (int64_t)H * W;
        float* gbase = grad + img * (int64_t)H * W;
        // every load of the strip is issued before the first use: the rows above, of and below the strip and the two neighbour columns,
        // at clamped -- always valid -- addresses (what a clamp made up is never used: the guards below are on the true indices)
        TvRow rows[kTvRows + 2];
        float lf[kTvRows], rt[kTvRows];
#pragma unroll
        for (int k = 0; k < kTvRows + 2; ++k) {
            int i = r0 - 1 + k;
            i = i < 0 ? 0 : (i > H - 1 ? H - 1 : i);
            rows[k] = tv_row<kVec>(base + (int64_t)i * W, c0, W);
        }
#pragma unroll
        for (int k = 0; k < kTvRows; ++k) {
            const int i = r0 + k < H ? r0 + k : H - 1;
            const float* row = base + (int64_t)i * W;
            lf[k] = row[c0 > 0 ? c0 - 1 : 0];
            rt[k] = row[c0 + 4 < W ? c0 + 4 : W - 1];
        }
#pragma unroll
        for (int q = 0; q < kTvRows; ++q) {
            const int i = r0 + q;
            if (i >= r1) break;
            const TvRow &up = rows[q], &cur = rows[q + 1], &dn = rows[q + 2];
            const double left = lf[q], right = rt[q];
            float out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + k;
                const double m = cur.v[k];
                double gv = 0.0, gh = 0.0;
                if (i > 0) gv += sl1_d(m - (double)up.v[k], kBeta);
                if (i + 1 < H) { const double x = (double)dn.v[k] - m; gv -= sl1_d(x, kBeta); if (c < W) sv += sl1(x, kBeta); }
                if (c > 0) gh += sl1_d(m - (k > 0 ? (double)cur.v[k - 1] : left), kBeta);
                if (c + 1 < W) { const double x = (k < 3 ? (double)cur.v[k + 1] : right) - m; gh -= sl1_d(x, kBeta); sh += sl1(x, kBeta); }
                out[k] = (float)(weight * (gv * inv_nv + gh * inv_nh));
            }
            if (kVec) {
                f32x4 v; v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3];
                *reinterpret_cast<f32x4*>(gbase + (int64_t)i * W + c0) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < W) gbase[(int64_t)i * W + c0 + k] = out[k];
            }
        }
    }
    const double tv = block_sum(sv, part), th = block_sum(sh, part);
    if (threadIdx.x == 0) { partials[2 * (int64_t)blockIdx.x] = tv; partials[2 * (int64_t)blockIdx.x + 1] = th; }
}

__global__ __launch_bounds__(kJtBlock) void joint_tv_finish_kernel(const double* __restrict__ partials, int n_blocks, double inv_nv, double inv_nh,
                                                                   float* __restrict__ value_out) {
    __shared__ double part[kJtBlock];
    double sv = 0.0, sh = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += kJtBlock) { sv += partials[2 * (int64_t)b]; sh += partials[2 * (int64_t)b + 1]; }
    const double tv = block_sum(sv, part), th = block_sum(sh, part);
    if (threadIdx.x == 0) value_out[0] = (float)(tv * inv_nv + th * inv_nh);
}

// what the two per-sample entry points refuse, in one place
static int check_joint(const char* who, int32_t P, int64_t B, int32_t R, int32_t Rn) {
    PERF_REQUIRE(P >= 0 && B >= 0, "%s: a negative count (P %d, B %lld)", who, (int)P, (long long)B);
    PERF_REQUIRE(P >= 1 && B >= 1, "%s: an empty step (P %d, B %lld): an alignment step has samples", who, (int)P, (long long)B);
    PERF_REQUIRE(B <= ((int64_t)1 << 30) / P, "%s: P * B exceeds 2^30", who);
    PERF_REQUIRE(B <= ((int64_t)1 << 20), "%s: B exceeds 2^20 samples per view", who);
    PERF_REQUIRE(R >= 1 && Rn >= 1, "%s: a map without texels (R %d, Rn %d)", who, (int)R, (int)Rn);
    return PERF_OK;
}

static int64_t tv_blocks(int64_t n, int32_t C, int32_t H, int32_t W) {
    const int64_t items = n * C * div_up(H, kTvRows) * div_up(W, 4);
    const int64_t blocks = div_up(items, kJtBlock);
    return blocks < kTvMaxBlocks ? blocks : kTvMaxBlocks;
}

static int check_tv(const char* who, int64_t n, int32_t C, int32_t H, int32_t W) {
    PERF_REQUIRE(n >= 0 && C >= 0 && H >= 0 && W >= 0, "%s: a negative count (n %lld, C %d, H %d, W %d)", who, (long long)n, (int)C, (int)H, (int)W);
    PERF_REQUIRE(n >= 1 && C >= 1, "%s: an empty map (n %lld, C %d)", who, (long long)n, (int)C);
    PERF_REQUIRE(H >= 2 && W >= 2, "%s: H and W must be at least 2 (H %d, W %d): the mean over no differences is not defined", who, (int)H, (int)W);
    PERF_REQUIRE(n <= ((int64_t)1 << 40) / ((int64_t)C * H * W), "%s: the map exceeds 2^40 entries", who);
    return PERF_OK;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_joint_version(void) { return PERF_JOINT_ABI_VERSION; }

extern "C" int perf_joint_sample(const float* sup, const float* bias_d, const float* bias_n, const float* ref, const float* coords,
                                 const float* u_given_or_null, int32_t P, int64_t B, int32_t R, int32_t Rn, int32_t H, int32_t W, float* u,
                                 float* rec, void* stream) {
    int rc = check_joint("perf_joint_sample", P, B, R, Rn);
    if (rc) return rc;
    PERF_REQUIRE(H >= 1 && W >= 1, "perf_joint_sample: a panorama without texels (H %d, W %d)", (int)H, (int)W);
    PERF_REQUIRE(sup && bias_d && bias_n && ref && coords, "perf_joint_sample: NULL input pointer");
    PERF_REQUIRE((u || u_given_or_null) && rec, "perf_joint_sample: NULL output pointer");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 15) == 0, "perf_joint_sample: the record must be 16-byte aligned");
    const int64_t N = (int64_t)P * B;
    joint_sample_kernel<<<dim3((unsigned)div_up(N, kJtBlock)), dim3(kJtBlock), 0, as_stream(stream)>>>(sup, bias_d, bias_n, ref, coords, u_given_or_null, N, B, R, Rn, H, W, u, rec);
    PERF_LAUNCH_CHECK("perf_joint_sample");
    return PERF_OK;
}

extern "C" int64_t perf_joint_loss_workspace_bytes(int32_t P, int64_t B) {
    if (check_joint("perf_joint_loss_workspace_bytes", P, B, 1, 1)) return -1;
    const int64_t N = (int64_t)P * B;
    return div_up((4 * div_up(N, kJtBlock) + N) * (int64_t)sizeof(double), 16) * 16;
}

extern "C" int perf_joint_loss(const float* rec, const float* coords, const float* scale, const float* u, const float* d, const float* g,
                               const float* o, int32_t P, int64_t B, int32_t R, int32_t Rn, float w_ref, float w_reg, float w_n, float w_ntv,
                               const float* tv_or_null, float* losses, float* dd, float* dg, float* dscale, float* gbias_d_or_null,
                               float* gbias_n_or_null, void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_joint("perf_joint_loss", P, B, R, Rn);
    if (rc) return rc;
    PERF_REQUIRE(rec && coords && scale && u && d && g && o, "perf_joint_loss: NULL input pointer");
    PERF_REQUIRE(losses && dd && dg && dscale, "perf_joint_loss: NULL output pointer");
    PERF_REQUIRE((gbias_d_or_null == nullptr) == (gbias_n_or_null == nullptr), "perf_joint_loss: the two map gradients come together (both or neither)");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 15) == 0, "perf_joint_loss: the record must be 16-byte aligned");
    PERF_REQUIRE(workspace != nullptr, "perf_joint_loss: NULL workspace");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "perf_joint_loss: the workspace must be 16-byte aligned");
    const int64_t need = perf_joint_loss_workspace_bytes(P, B);
    PERF_REQUIRE(workspace_bytes >= need, "perf_joint_loss: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    JointLossArgs A;
    A.rec = rec; A.coords = coords; A.scale = scale; A.u = u; A.d = d; A.g = g; A.o = o; A.tv = tv_or_null;
    A.losses = losses; A.dd = dd; A.dg = dg; A.dscale = dscale; A.gbias_d = gbias_d_or_null; A.gbias_n = gbias_n_or_null;
    A.N = (int64_t)P * B; A.B = B; A.P = P; A.R = R; A.Rn = Rn;
    A.n_blocks = (int)div_up(A.N, kJtBlock);
    A.partials = (double*)workspace;
    A.contrib = A.partials + 4 * (int64_t)A.n_blocks;
    A.w_ref = w_ref; A.w_reg = w_reg; A.w_n = w_n; A.w_ntv = w_ntv;
    const hipStream_t st = as_stream(stream);
    joint_loss_kernel<<<dim3((unsigned)A.n_blocks), dim3(kJtBlock), 0, st>>>(A);
    PERF_LAUNCH_CHECK("perf_joint_loss");
    joint_loss_finish_kernel<<<dim3(1), dim3(kJtBlock), 0, st>>>(A);
    PERF_LAUNCH_CHECK("perf_joint_loss(finish)");
    return PERF_OK;
}

extern "C" int64_t perf_joint_tv_workspace_bytes(int64_t n, int32_t C, int32_t H, int32_t W) {
    if (check_tv("perf_joint_tv_workspace_bytes", n, C, H, W)) return -1;
    return (int64_t)kTvMaxBlocks * 2 * (int64_t)sizeof(double);
}

extern "C" int perf_joint_tv(const float* map, int64_t n, int32_t C, int32_t H, int32_t W, float weight, float* grad_out, float* value_out,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_tv("perf_joint_tv", n, C, H, W);
    if (rc) return rc;
    PERF_REQUIRE(map != nullptr, "perf_joint_tv: NULL input pointer");
    PERF_REQUIRE(grad_out && value_out, "perf_joint_tv: NULL output pointer");
    PERF_REQUIRE(workspace != nullptr, "perf_joint_tv: NULL workspace");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "perf_joint_tv: the workspace must be 16-byte aligned");
    const int64_t need = perf_joint_tv_workspace_bytes(n, C, H, W);
    PERF_REQUIRE(workspace_bytes >= need, "perf_joint_tv: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    const int64_t n_img = n * C;
    const int blocks = (int)tv_blocks(n, C, H, W);
    const double inv_nv = 1.0 / ((double)n_img * (H - 1) * W), inv_nh = 1.0 / ((double)n_img * H * (W - 1));
    const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(map) | reinterpret_cast<uintptr_t>(grad_out)) & 15) == 0;
    const hipStream_t st = as_stream(stream);
    double* partials = (double*)workspace;
    if (vec)
        joint_tv_kernel<true><<<dim3((unsigned)blocks), dim3(kJtBlock), 0, st>>>(map, grad_out, n_img, H, W, (double)weight, inv_nv, inv_nh, partials);
    else
        joint_tv_kernel<false><<<dim3((unsigned)blocks), dim3(kJtBlock), 0, st>>>(map, grad_out, n_img, H, W, (double)weight, inv_nv, inv_nh, partials);
    PERF_LAUNCH_CHECK("perf_joint_tv");
    joint_tv_finish_kernel<<<dim3(1), dim3(kJtBlock), 0, st>>>(partials, blocks, inv_nv, inv_nh, value_out);
    PERF_LAUNCH_CHECK("perf_joint_tv(finish)");
    return PERF_OK;
}
