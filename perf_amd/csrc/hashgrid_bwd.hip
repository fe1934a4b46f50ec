// Hash-grid parameter gradient for gfx950 (tcnn kernel_grid_backward semantics): LDS tile owners, no global atomics.
#include <stdlib.h>
#include <mutex>
#include "common.hpp"
#include "grid_device.hpp"
#include "grid_fixed_point.hpp"
#include "mlp_reduce_device.hpp"
#include "step_book_device.hpp"
#include "step_riders_device.hpp"

namespace perf {

// Parameter gradient.  gfx950 global fp32 atomics retire at a flat ~2e10/s whatever their scope or
// address distribution (tools/exp/atomics.hip), i.e. ~13 ms for the 2.7e8 corner updates of a
// 1 M-sample batch -- so the scatter is turned inside out: the fp32 gradient table (26.6 MB for
// L16/T18) is cut into 128 KiB tiles of 16384 entries and each tile is OWNED by one workgroup that
// keeps it in LDS (the multi-tile levels' 192 + 12 tiles plus the replicated coarse ones <= 256 CUs: the whole
// table is resident in the chip's aggregate LDS).  Every owner walks all samples of its level and applies only the
// corner updates that fall in its tile with LDS atomics -- multi-tile levels through a tile code per sample that a
// pre-pass computes once for all owners (hashed levels of up to 16 tiles: one bit row per tile, bwd_stream_bits; others:
// 4 bytes per sample, bwd_stream_codes), single-tile levels from positions (bwd_stream);
// at the end the tile is written back with plain coalesced stores.  No global atomics, no zero-fill pass, every
// table entry written exactly once.
constexpr int kTileEntries = 16384;
constexpr int kBwdThreads = 1024;
constexpr int kMaxReplicas = 16;
constexpr int kMaxWork = 512;              // workgroups the XCD-aware placement table can hold
constexpr int kXcds = 8;
constexpr int kCus = 248;                  // MI355X has 256 CUs and an owner workgroup (128 KiB of LDS) takes one -- but a launch of 252 did not get
                                           // one each: 731 us against 361 (call r06cu); 31 per XCD is what is asked for at most

// Load balance: a hashed level has 16 tiles, each receiving 1/16 of the level's 8 corner updates per
// sample; a coarse dense level has only 1..8 tiles receiving the same total.  Coarse tiles are therefore
// REPLICATED (R_l copies, each streaming 1/R_l of the samples) so that every workgroup takes about as long as
// a hashed-tile owner; replicas are summed by a small second kernel.  L16/T18, fixed-point mode:
// 8 + 8 + 4x4 + 8x3 + 12x16 = 248 workgroups (the third replica of level 3 and the fourth of level 2 from the CUs left over, see plan_tiles).
struct TileParams {
    int32_t tiles_of[PERF_MAX_LEVELS];     // tiles per level
    int32_t replicas_of[PERF_MAX_LEVELS];  // replicas per tile
    int64_t ws_off[PERF_MAX_LEVELS];       // float2 offset of the level's replica slabs in the workspace
    int32_t accumulate;
    int32_t code_slot[PERF_MAX_LEVELS];    // >=0: the level's tile codes are codes[slot][n_pad] (see tile_codes4_kernel)
    int64_t n_pad;
    // XCD-aware placement: workgroup b runs work[b] = level << 16 | tile << 8 | replica (0xffffffff: idle).  The
    // dispatcher deals workgroups round-robin over the 8 XCDs, so b % 8 is the XCD: the owners of one level are put on
    // the same XCD -- they stream the same codes and gather the same position / gradient lines at about the same
    // time, which then hit that XCD's L2 instead of crossing the fabric 16 times.  use_work == 0: plain level order.
    int32_t use_work;
    int32_t raw_out;                       // fixed point: the gradient table receives the int32 field pairs themselves (see perf_hashgrid_bwd)
    uint32_t atomic_levels;                // bit l: level l is too large for LDS owners (see hashgrid_bwd_atomic_kernel)
    uint32_t bitmap_levels;                // bit l: hashed level of 256..kBitmapMaxTiles tiles whose owners read per-tile bitmaps (tile_bitmap_kernel)
    int32_t bm_row[PERF_MAX_LEVELS];       // first bitmap row (= tile 0) of such a level, its index among them in bm_idx
    int32_t bm_idx[PERF_MAX_LEVELS];
    int64_t bm_row_words;                  // 32-bit words per bitmap row (bm_samples / 32 per pre-pass block)
    int64_t bm_blocks;                     // pre-pass blocks = escape words per bitmap level
    int32_t bm_samples;                    // samples per pre-pass block (256..1024: tiles x bm_samples / 8 bytes of LDS staging <= 64 KiB)
    int32_t run_merge;                     // single-tile dense levels: a thread sums runs of samples in one cell in registers
    uint32_t work[kMaxWork];
};

// per-wave match queue (entries).  (The bit-row owners state their own count beside bwd_stream_bits.)  An iteration of the code loop starts with fewer than 128 entries (its burst loop ran
// until then; the first starts empty), its four enqueue rounds add at most 4 x 64 (one per lane and sample slot: < 384), the apply's
// re-queue at most 64 (< 448); the pop that follows takes 64 of them when there are that many, and every further burst round pops as
// many as its apply re-queues at most.
constexpr int kQueueCap = 448;
// Levels whose owners stream tile codes (plan_codes): at most this many tiles.  Their owners form indices with the full-rate 24-bit
// multiplier, which is exact while an index of the level fits 24 bits.
constexpr int kMaxCodedHashedTiles = 255, kMaxCodedDenseTiles = 64;
static_assert((int64_t)(kMaxCodedHashedTiles + 1) * 16384 <= ((int64_t)1 << 24) && (int64_t)kMaxCodedDenseTiles * 16384 <= ((int64_t)1 << 24),
              "coded levels: indices must fit 24 bits (bwd_stream_bits / bwd_stream_codes multiply with v_mul_u32_u24)");
constexpr int64_t kMaxCodedSamples = (int64_t)1 << 28;

constexpr int kBitmapMinDenseTiles = 32;
constexpr int kBitmapMaxTiles = 2048;      // (2048 x 32 bytes of LDS staging per pre-pass block; log2_hashmap_size <= 25)

// bitmap_tiles > 0: hashed levels of 256..bitmap_tiles tiles get LDS owners fed by per-tile bitmaps instead of the global
// atomics (the caller checks that the workspace holds the bitmaps and plans again with 0 otherwise)
static void plan_tiles(const GridParams& gp, bool fixed, TileParams* tp, int* n_blocks, int64_t* ws_entries, int bitmap_tiles = 0,
                       bool no_replicas = false) {
    int nb = 0;
    int64_t ws = 0;
    tp->atomic_levels = 0u;
    tp->bitmap_levels = 0u;
    const int rs[3] = {8, 3, 2};       // replicas of dense levels of 1 / <= 4 / <= 16 tiles
    bool large_grid = false;        // some level takes bitmap owners
    for (int l = 0; l < gp.n_levels && bitmap_tiles > 0; ++l) {
        int nt = (int)((gp.size[l] + kTileEntries - 1) / kTileEntries);
        if (!gp.hashed[l]) { int p2 = 1; while (p2 < nt) p2 <<= 1; nt = p2; }
        if (nt <= bitmap_tiles && (gp.hashed[l] ? (nt > 255 && gp.res[l] + 2u < (uint32_t)kTileEntries) : nt >= kBitmapMinDenseTiles)) large_grid = true;
    }
    for (int l = 0; l < PERF_MAX_LEVELS; ++l) {
        tp->tiles_of[l] = 0; tp->replicas_of[l] = 1; tp->ws_off[l] = 0;
        if (l >= gp.n_levels) continue;
        int nt = (int)((gp.size[l] + kTileEntries - 1) / kTileEntries);
        if (!gp.hashed[l]) { int p = 1; while (p < nt) p <<= 1; nt = p; }     // dense ownership is a bit field of the index
        // A level of more than 255 (hashed) / 64 (dense) tiles = 4 M / 1 M entries would need that many owners, each
        // walking every sample: beyond that the plain global-atomics scatter is cheaper (log2_hashmap_size >= 22).
        // (dense levels already from 32 tiles: a sample touches 4-5 of them, and code-streaming owners that each test every
        //  sample are the long pole of a 20-level grid -- 1.6 ms per 1 M random points at 64 tiles)
        if (nt > (gp.hashed[l] ? 255 : 64) || (!gp.hashed[l] && nt >= kBitmapMinDenseTiles && nt <= bitmap_tiles)) {
            if (nt <= bitmap_tiles && (!gp.hashed[l] || gp.res[l] + 2u < (uint32_t)kTileEntries)) {
                tp->bitmap_levels |= 1u << l;
                tp->tiles_of[l] = nt;
                nb += nt;
            } else {
                tp->atomic_levels |= 1u << l;
            }
            continue;
        }
        // replication factors from measured per-workgroup times (tools/exp/bwd_block_times.py, 1 M samples, fixed):
        // hashed tile (coded) 0.36-0.39 ms; dense tile streaming ALL samples: 1 tile 2.4 ms, 4 tiles 0.88 ms, 8 tiles 0.68 ms
        // (fp32 mode is bound by ds_add_f32 lane-serialisation instead: equal corner-update counts, r = 16 / nt)
        int r = 1;
        if (!gp.hashed[l]) r = fixed ? ((nt == 1) ? rs[0] : (nt <= 4 ? rs[1] : (nt <= 16 ? rs[2] : 1))) : kMaxReplicas / nt;
        // A grid with bitmap levels launches thousands of short owners anyway: its few-tile dense levels -- where every sample
        // is an entry of most owners -- get the replicas that keep them from being the kernel's long pole (measured on a
        // 20-level grid: 2 tiles x 3 replicas 1.1 ms per workgroup, 8 x 2 0.66 ms, against 0.07-0.3 ms everywhere else)
        if (!gp.hashed[l] && fixed && bitmap_tiles > 0 && large_grid) r = nt == 1 ? 8 : (nt == 2 ? 8 : (nt == 4 ? 6 : (nt == 8 ? 4 : 2)));
        if (r < 1 || no_replicas) r = 1;
        if (r > kMaxReplicas) r = kMaxReplicas;
        tp->tiles_of[l] = nt; tp->replicas_of[l] = r;
        if (r > 1) { tp->ws_off[l] = ws; ws += (int64_t)r * gp.size[l]; }
        nb += nt * r;
    }
    // ---- CUs left over go to the dense levels of 5..16 tiles (round 6, per-workgroup times of a 1 M-sample call: the 8 tiles x 2
    // replicas of level 3 of L16 / T18 took 357 us each, every hashed owner 331-350 -- the launch ended with them; 16 of the 20 idle CUs
    // as two more replicas bring them to ~190).  Only while the launch still fits one workgroup per CU, and only in fixed-point mode
    // (integer slabs: the sums do not depend on how the samples are split).
    if (fixed && !no_replicas && !large_grid && tp->bitmap_levels == 0u && tp->atomic_levels == 0u) {
        for (int want = 4; want >= 3; --want)
            for (int l = 0; l < gp.n_levels; ++l) {
                const int nt = tp->tiles_of[l], r = tp->replicas_of[l];
                if (gp.hashed[l] || nt <= 4 || nt > 16 || r != rs[2] || want <= r) continue;
                if (nb + nt * (want - r) > kCus) continue;
                nb += nt * (want - r);
                tp->replicas_of[l] = want;
            }
        // ---- and then to the dense levels of 2..4 tiles.  With the hashed owners on 16-bit tile masks (283-306 us per workgroup, were
        // 297-335) the 4 tiles x 3 replicas of level 2 of L16 / T18 ended the launch at 342 us; a fourth replica brings them to 268 and
        // the launch from 331 to 316 us on one box (profiles/bwd_tile_masks.json; 248 workgroups = kCus).  With the hashed owners on bit
        // rows (bwd_stream_bits) every kind of workgroup of the bench step takes 238-250 us (profiles/bwd_bit_rows.json: hashed 238-250,
        // level 2's 4 x 4 250, the single-tile levels' 8 replicas 245, level 3's 8 x 3 238): the launch ends with all of them at once,
        // there is no CU left (kCus), and no replica count is changed.  (Round 6
        // measured the same replica as a LOSS, 357.0 against 352.5 us: the hashed owners ended the launch then, and four more neighbours
        // cost them more than level 2 gained.)  Only while its slab fits the room the fp32 plan's slabs take anyway (16 / tiles replicas):
        // the workspace a grid asks for stays what it was.
        int64_t ws_fixed = 0, ws_fp32 = 0;
        for (int l = 0; l < gp.n_levels; ++l) {
            const int nt = tp->tiles_of[l];
            if (tp->replicas_of[l] > 1) ws_fixed += (int64_t)tp->replicas_of[l] * gp.size[l];
            if (!gp.hashed[l] && nt > 0 && kMaxReplicas / nt > 1) ws_fp32 += (int64_t)(kMaxReplicas / nt) * gp.size[l];
        }
        for (int l = 0; l < gp.n_levels; ++l) {
            const int nt = tp->tiles_of[l], r = tp->replicas_of[l];
            if (gp.hashed[l] || nt < 2 || nt > 4 || r != rs[1] || nb + nt > kCus || ws_fixed + (int64_t)gp.size[l] > ws_fp32) continue;
            nb += nt;
            ws_fixed += gp.size[l];
            tp->replicas_of[l] = r + 1;
        }
        ws = 0;                                              // (slab offsets again)
        for (int l = 0; l < gp.n_levels; ++l) {
            tp->ws_off[l] = 0;
            if (tp->replicas_of[l] > 1) { tp->ws_off[l] = ws; ws += (int64_t)tp->replicas_of[l] * gp.size[l]; }
        }
    }
    *n_blocks = nb; *ws_entries = ws;
    // ---- XCD-aware placement (a speed assumption only: results do not depend on it)
    tp->use_work = 0;
    if (nb > kMaxWork || tp->bitmap_levels) return;       // (the table packs the tile in 8 bits)
    uint32_t lists[kXcds][kMaxWork];                        // 16 KiB of stack: the planner is re-entrant
    int len[kXcds] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto least = [&]() { int x = 0; for (int i = 1; i < kXcds; ++i) if (len[i] < len[x]) x = i; return x; };
    const int per_xcd = (nb + kXcds - 1) / kXcds;
    for (int pass = 0; pass < 2; ++pass)                    // multi-tile levels first (they are the ones that share), then the rest
        for (int l = gp.n_levels - 1; l >= 0; --l) {
            const int nt = tp->tiles_of[l], R = tp->replicas_of[l];
            if ((nt > 1) != (pass == 0)) continue;
            int x = least();
            for (int t = 0; t < nt; ++t)
                for (int r = 0; r < R; ++r) {
                    if (len[x] >= per_xcd) x = least();     // the level spills over to the emptiest XCD
                    lists[x][len[x]++] = ((uint32_t)l << 16) | ((uint32_t)t << 8) | (uint32_t)r;
                }
        }
    int longest = 0;
    for (int x = 0; x < kXcds; ++x) longest = len[x] > longest ? len[x] : longest;
    if (longest * kXcds > kMaxWork) return;
    for (int slot = 0; slot < longest; ++slot)
        for (int x = 0; x < kXcds; ++x) tp->work[slot * kXcds + x] = slot < len[x] ? lists[x][slot] : 0xffffffffu;
    tp->use_work = 1;
    *n_blocks = longest * kXcds;
}

// Tile ownership.  Hashed levels: tile = idx / 16384 (the hash already spreads cells uniformly).  Dense levels:
// ownership is INTERLEAVED in chunks of 32 entries over a power-of-two number of tiles (chunk c = idx/32 belongs
// to tile c % n_tiles, local slot (c / n_tiles)*32 + idx%32) -- contiguous slabs would be spatial slabs, and samples concentrate near the
// camera / the surfaces, which overloads a few owners.
constexpr uint32_t kChunk = 32;

struct BwdCtx {
    float scale, to_fixed;
    uint32_t res, r2, size, mask, n_tiles, t;
    uint32_t tile_shift;        // dense levels: log2(n_tiles)
    bool smooth;
};

// (y,z)-combination updates of one sample in a hashed tile: both x-corners of every combination in `cm`
// (bit c: by = c & 1, bz = c >> 1).  Requires gx + 1 < kTileEntries (the tile then depends on (y,z) only).
template <bool FIXED>
__device__ __forceinline__ void apply_pairs(const BwdCtx& cx, float* lds_tile, const float2 g, const uint32_t gx, float fx,
                                            float fy, float fz, const uint32_t ay0, const uint32_t az0, uint32_t cm) {
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds_tile);
    if (cx.smooth) { fx = fx * fx * (3.0f - 2.0f * fx); fy = fy * fy * (3.0f - 2.0f * fy); fz = fz * fz * (3.0f - 2.0f * fz); }
    const uint32_t tlo = cx.t * (uint32_t)kTileEntries;
    const float sx = g.x * cx.to_fixed, sy = g.y * cx.to_fixed;
    while (cm) {
        const int c = __ffs(cm) - 1;
        cm &= cm - 1u;
        const int by = c & 1, bz = c >> 1;
        const uint32_t h = (by ? ay0 + kPrimeY : ay0) ^ (bz ? az0 + kPrimeZ : az0);
        const float wyz = (by ? fy : 1.0f - fy) * (bz ? fz : 1.0f - fz);
        const uint32_t a0 = ((gx ^ h) & cx.mask) - tlo, a1 = (((gx + 1u) ^ h) & cx.mask) - tlo;
        const float w0 = (1.0f - fx) * wyz, w1 = fx * wyz;
        if (FIXED) {
            const long long v0 = ((long long)__float2int_rn(w0 * sy) << 32) + (long long)__float2int_rn(w0 * sx);
            const long long v1 = ((long long)__float2int_rn(w1 * sy) << 32) + (long long)__float2int_rn(w1 * sx);
            atomicAdd(&lds64[a0], (unsigned long long)v0);
            atomicAdd(&lds64[a1], (unsigned long long)v1);
        } else {
            unsafeAtomicAdd(&lds_tile[2 * a0], w0 * g.x); unsafeAtomicAdd(&lds_tile[2 * a0 + 1], w0 * g.y);
            unsafeAtomicAdd(&lds_tile[2 * a1], w1 * g.x); unsafeAtomicAdd(&lds_tile[2 * a1 + 1], w1 * g.y);
        }
    }
}

// (hi << 32) + lo of two signed fields as one 64-bit word, in 32-bit instructions: the sign extension of lo takes one from hi
__device__ __forceinline__ unsigned long long field_pair(int lo, int hi) {
    return ((unsigned long long)((uint32_t)hi + (uint32_t)(lo >> 31)) << 32) | (unsigned long long)(uint32_t)lo;
}

// The same for ONE combination (`cm` has exactly one bit set): what the code and mask owners pass, every lane its lowest.  Straight
// line -- no find-first-bit, no loop mask, no back edge --, the factors of apply_pairs in its order: its sums to the bit.
template <bool FIXED>
__device__ __forceinline__ void apply_pair_one(const BwdCtx& cx, float* lds_tile, const float2 g, const uint32_t gx, float fx,
                                               float fy, float fz, const uint32_t ay0, const uint32_t az0, const uint32_t cm) {
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds_tile);
    if (cx.smooth) { fx = fx * fx * (3.0f - 2.0f * fx); fy = fy * fy * (3.0f - 2.0f * fy); fz = fz * fz * (3.0f - 2.0f * fz); }
    const uint32_t tlo = cx.t * (uint32_t)kTileEntries;
    const float sx = g.x * cx.to_fixed, sy = g.y * cx.to_fixed;
    const bool by = (cm & 0xau) != 0u, bz = (cm & 0xcu) != 0u;
    const uint32_t h = (by ? ay0 + kPrimeY : ay0) ^ (bz ? az0 + kPrimeZ : az0);
    const float wyz = (by ? fy : 1.0f - fy) * (bz ? fz : 1.0f - fz);
    const uint32_t a0 = ((gx ^ h) & cx.mask) - tlo, a1 = (((gx + 1u) ^ h) & cx.mask) - tlo;
    const float w0 = (1.0f - fx) * wyz, w1 = fx * wyz;
    if (FIXED) {
        atomicAdd(&lds64[a0], field_pair(__float2int_rn(w0 * sx), __float2int_rn(w0 * sy)));
        atomicAdd(&lds64[a1], field_pair(__float2int_rn(w1 * sx), __float2int_rn(w1 * sy)));
    } else {
        unsafeAtomicAdd(&lds_tile[2 * a0], w0 * g.x); unsafeAtomicAdd(&lds_tile[2 * a0 + 1], w0 * g.y);
        unsafeAtomicAdd(&lds_tile[2 * a1], w1 * g.x); unsafeAtomicAdd(&lds_tile[2 * a1 + 1], w1 * g.y);
    }
}

// Dense-level counterpart (interleaved 32-entry chunks): the two x-corners of a (y,z) combination are tested
// separately -- they part at a chunk boundary -- and a combination that would wrap past the end of the level
// (position far outside the unit cube; such a level takes the generic owners, see tile_codes4_kernel) is skipped.
// ay0 / az0 need only be right in their low 24 bits (bwd_stream_codes forms them with the 24-bit multiplier): the pre-pass names a tile
// only for a sample all of whose x0 corners lie below size - 1 <= 2^20 in exact 32-bit arithmetic (any 0x7f byte sends the sample to
// bwd_apply), so the low 24 bits of the sum ARE the index.
template <bool FIXED>
__device__ __forceinline__ void apply_pairs_dense(const BwdCtx& cx, float* lds_tile, const float2 g, const uint32_t gx, float fx,
                                                  float fy, float fz, const uint32_t ay0, const uint32_t az0, uint32_t cm) {
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds_tile);
    if (cx.smooth) { fx = fx * fx * (3.0f - 2.0f * fx); fy = fy * fy * (3.0f - 2.0f * fy); fz = fz * fz * (3.0f - 2.0f * fz); }
    const float sx = g.x * cx.to_fixed, sy = g.y * cx.to_fixed;
    const uint32_t tmask = cx.n_tiles - 1u;
    while (cm) {
        const int c = __ffs(cm) - 1;
        cm &= cm - 1u;
        const int by = c & 1, bz = c >> 1;
        const uint32_t i0 = (gx + (by ? ay0 + cx.res : ay0) + (bz ? az0 + cx.r2 : az0)) & 0xffffffu, i1 = i0 + 1u;
        if (i1 >= cx.size || i1 == 0u) continue;
        const float wy = by ? fy : 1.0f - fy, wz = bz ? fz : 1.0f - fz;
        const float w0 = ((1.0f - fx) * wy) * wz, w1 = (fx * wy) * wz;      // association of the generic owners
        const uint32_t c0 = i0 / kChunk, c1 = i1 / kChunk;
        const uint32_t a0 = (c0 >> cx.tile_shift) * kChunk + (i0 % kChunk), a1 = (c1 >> cx.tile_shift) * kChunk + (i1 % kChunk);
        if ((c0 & tmask) == cx.t) {
            if (FIXED) atomicAdd(&lds64[a0], field_pair(__float2int_rn(w0 * sx), __float2int_rn(w0 * sy)));
            else { unsafeAtomicAdd(&lds_tile[2 * a0], w0 * g.x); unsafeAtomicAdd(&lds_tile[2 * a0 + 1], w0 * g.y); }
        }
        if ((c1 & tmask) == cx.t) {
            if (FIXED) atomicAdd(&lds64[a1], field_pair(__float2int_rn(w1 * sx), __float2int_rn(w1 * sy)));
            else { unsafeAtomicAdd(&lds_tile[2 * a1], w1 * g.x); unsafeAtomicAdd(&lds_tile[2 * a1 + 1], w1 * g.y); }
        }
    }
}

// one sample's contribution to the tile this workgroup owns
template <bool FIXED, bool HASHED>
__device__ __forceinline__ void bwd_apply(const BwdCtx& cx, float* lds_tile, const float2 g, const float x, const float y,
                                          const float z) {
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds_tile);
    const float px = grid_pos(x, cx.scale), py = grid_pos(y, cx.scale), pz = grid_pos(z, cx.scale);
    const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
    float fx = px - flx, fy = py - fly, fz = pz - flz;
    const uint32_t gx = (uint32_t)(int32_t)flx, gy = (uint32_t)(int32_t)fly, gz = (uint32_t)(int32_t)flz;
    uint32_t ay[2], az[2];
    uint32_t match = 0;     // bit k: corner k (bit0 = x, bit1 = y, bit2 = z) is owned by this tile
    if (HASHED) {
        ay[0] = gy * kPrimeY; ay[1] = ay[0] + kPrimeY; az[0] = gz * kPrimeZ; az[1] = az[0] + kPrimeZ;
        if (gx < (uint32_t)(kTileEntries - 1)) {
            // The tile of a hashed corner depends on (y,z) only while gx+1 < 2^14, so the two x-corners of a (y,z)
            // combination are tested and applied together: 4 tests and at most 4 (usually 0-1) pair updates.
            uint32_t cm = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                cm |= (((((ay[c & 1] ^ az[c >> 1]) & cx.mask) / (uint32_t)kTileEntries) == cx.t) ? 1u : 0u) << c;
            if (cm == 0) return;
            apply_pairs<FIXED>(cx, lds_tile, g, gx, fx, fy, fz, ay[0], az[0], cm);
            return;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t idx = ((gx + (uint32_t)(k & 1)) ^ ay[(k >> 1) & 1] ^ az[k >> 2]) & cx.mask;
            match |= ((idx / (uint32_t)kTileEntries) == cx.t ? 1u : 0u) << k;
        }
    } else {
        ay[0] = gy * cx.res; ay[1] = ay[0] + cx.res; az[0] = gz * cx.r2; az[1] = az[0] + cx.r2;
        if (cx.n_tiles == 1) match = 0xffu;
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t idx = (gx + (uint32_t)(k & 1)) + ay[(k >> 1) & 1] + az[k >> 2];
                if (idx >= cx.size) idx = idx % cx.size;
                match |= (((idx / kChunk) & (cx.n_tiles - 1u)) == cx.t ? 1u : 0u) << k;
            }
        }
    }
    if (match == 0) return;
    if (cx.smooth) { fx = fx * fx * (3.0f - 2.0f * fx); fy = fy * fy * (3.0f - 2.0f * fy); fz = fz * fz * (3.0f - 2.0f * fz); }
    while (match) {
        const int k = __ffs(match) - 1;
        match &= match - 1u;
        const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
        const uint32_t cy = by ? ay[1] : ay[0], cz = bz ? az[1] : az[0];
        uint32_t a;
        if (HASHED) a = (((gx + (uint32_t)bx) ^ cy ^ cz) & cx.mask) - cx.t * (uint32_t)kTileEntries;
        else {
            uint32_t idx = (gx + (uint32_t)bx) + cy + cz;
            if (idx >= cx.size) idx = idx % cx.size;
            a = ((idx / kChunk) >> cx.tile_shift) * kChunk + (idx % kChunk);
        }
        const float w = ((bx ? fx : 1.0f - fx) * (by ? fy : 1.0f - fy)) * (bz ? fz : 1.0f - fz);
        if (FIXED) {
            const long long lo = (long long)__float2int_rn(w * g.x * cx.to_fixed);
            const long long hi = (long long)__float2int_rn(w * g.y * cx.to_fixed);
            atomicAdd(&lds64[a], (unsigned long long)((hi << 32) + lo));
        } else {
            unsafeAtomicAdd(&lds_tile[2 * a], w * g.x);
            unsafeAtomicAdd(&lds_tile[2 * a + 1], w * g.y);
        }
    }
}


// ---- hashed owners, coded variant ------------------------------------------------------------------------------
// The owner test of a hashed level depends on (y,z) only, and it is the same for the 16 owners of the level, so a
// pre-pass (tile_codes4_kernel) evaluates it ONCE per (sample, level): one byte per (y,z) combination = the tile the
// combination's two x-corners fall in.  An owner then streams 4-byte codes instead of positions + gradients, keeps
// the samples that name its tile in a wave-private LDS queue (one ballot per sample) and applies them 64 at a time
// at full lane occupancy; positions and gradients are gathered for queued samples only (about 22 % of them), and the
// gather of one batch is issued one drain ahead of its use.
constexpr int kCodeSamplesPerBlock = 256;
// (Round 3 measured two ways of sparing the owners their tests, both bit-identical, neither kept -- tools/exp/bwd_sort.py,
//  profiles/r03_bwd_sorted_variants.json, r03_bwd_bitmap_variants.json, the code is in the history:
//  * counting-sorted per-tile record lists, so that an owner walks only its own records: the owners became GATHER bound
//    -- 0.37-0.43 ms per workgroup against 0.32; 0.164 ms with the gathers stubbed out -- because a list that is not in
//    sample order loses the 2-3 queued samples per 128-byte line that neighbouring lanes share, and the sort pass took
//    0.65 ms;
//  * one bit per (tile, sample) instead of the codes, expanded to queue entries with a wave scan: owners 0.325 ->
//    0.277 ms per workgroup, but the kernel ends with its burstiest level (0.31 ms) and the pre-pass grew by 0.085 ms -- four LDS
//    atomics per sample and level into a staged row.  Levels of at most 16 tiles have their bit rows now, from a transposition of
//    the masks in registers that costs the pre-pass 7 us: below.
//  What an owner costs is the drain: gather 20 B per queued sample, ~95 instructions and two 64-bit LDS atomics per
//  combination; tests, gathers and LDS are within 2x of each other, so removing one of them moves little.)

// Hashed levels of at most 16 tiles (log2_hashmap_size <= 18) keep one BIT ROW per tile instead of the four bytes per sample: row t
// has the bit of sample i set when any of the sample's four (y,z) combinations names tile t, so that an owner reads n / 8 bytes and
// pays per hit (bwd_stream_bits).  The pre-pass forms a 16-bit mask of the named tiles per sample in registers and transposes the
// masks of a DPP row of 16 lanes (64 samples) into 64 bits per tile (store_bit_rows): a workgroup writes a piece of 32 bytes per row,
// whole, so the rows need no zero fill.  The rows live in the level's code slot, row t at t * bit_row_words(n) words: 16 pieces of
// 32 bytes per block of 256 samples are 2 bytes per sample, what the masks took, but the last block's pieces are written whole -- up
// to 512 bytes of the slot's second half (a slot is 4 n_pad bytes and holds 512 * ceil(n / 256) for any n >= 256; below that a call's
// bit-row levels take the position-streaming owners, perf_internal_hashgrid_bwd_riders).
// Bit order, stated here once (bit_row_first_sample): a row is an array of 16-bit halfwords, halfword h holds the samples
// 64 * (h / 4) + (h % 4) + 4 * b in bit b = 0..15 -- slot k = h % 4 of the 16 lanes of DPP row h / 4 % 4 of the block's wave.  A
// halfword's hits stay inside a window of 64 samples, which keeps the gathers' line sharing.
constexpr int kMaskTiles = 16;
__device__ __forceinline__ uint32_t bit_row_first_sample(uint32_t h) { return ((h >> 2) << 6) | (h & 3u); }      // bit b: this + 4 b
__host__ __device__ inline int64_t bit_row_words(int64_t n) { return (n + kCodeSamplesPerBlock - 1) / kCodeSamplesPerBlock * (kCodeSamplesPerBlock / 32); }
constexpr uint32_t kCodeMasks = 0u, kCodeBytes = 1u, kCodeDense = 2u, kCodeDenseWide = 3u;
constexpr uint32_t kPackedMaxRes = 500;     // kCodeDense: res <= 500, so that no corner index of cells below 16383 wraps (16383 * (1 + 500 + 500^2) + 500 + 500^2 < 2^32)

// What the pre-pass needs of one coded level, as ONE 48-byte piece of the kernel arguments: two wide scalar loads per level,
// requested one level ahead.  (Read field by field out of GridParams / TileParams -- 3.4 KB by value -- a level cost three dependent
// scalar loads per SAMPLE, each waited for: profiles/tile_codes_prepass.json.)  Only coded levels are listed.
struct CodeLevel {
    float scale;
    uint32_t kind_level;        // kCode... | level << 8
    uint32_t last;              // size - 1: a hashed level's index mask; a dense level's last entry (an x0 corner there or beyond has no x1 corner)
    uint32_t res, res2;         // dense
    uint32_t tmask;             // dense: tiles - 1 (1..63: single-tile levels are not coded)
    int64_t row;                // slot * n_pad: the level's code row, in 4-byte words from `codes`
    // dense, one byte per (y,z) combination c, whose x0 corner lies off_c = (c & 1) * res + (c >> 1) * res2 entries after the sample's first:
    uint32_t off5;              // off_c % 32
    uint32_t offc;              // (off_c / 32) % 64
    uint32_t tmask4;            // tmask
    uint32_t pad;
};
constexpr int kCodeWaves = 4;   // waves of a pre-pass workgroup: wave w takes the listed levels w, w + 4, ...
struct CodePlan {
    CodeLevel lv[PERF_MAX_LEVELS + kCodeWaves];     // (the tail stays zero: a wave requests the descriptor after its last unconditionally)
    int32_t n_coded;
};

// Cell of a coordinate.  INSIDE: the caller knows that the grid position is >= 0 (or NaN), where the conversion's truncation IS the floor.
template <bool INSIDE>
__device__ __forceinline__ uint32_t code_cell(float v, float scale) {
    const float p = grid_pos(v, scale);
    return (uint32_t)(int32_t)(INSIDE ? p : floorf(p));
}

// The (y,z) part of a hashed level's four tile expressions.  A tile is bits 14 and up of an index below size <= 2^22 (coded levels
// have at most 255 tiles), so only the low 24 bits of gy * P_y and gz * P_z count, and those are the low 24 bits of the full-rate
// 24-bit product of the factors' low 24 bits: the same tiles as the 32-bit (quarter-rate) multiply gives, for any gy, gz.
template <bool INSIDE>
__device__ __forceinline__ void hashed_tiles(const CodeLevel& d, float y, float z, uint32_t t[4]) {
    const uint32_t gy = code_cell<INSIDE>(y, d.scale), gz = code_cell<INSIDE>(z, d.scale);
    const uint32_t ay0 = __umul24(gy, kPrimeY & 0xffffffu), ay1 = ay0 + kPrimeY, az0 = __umul24(gz, kPrimeZ & 0xffffffu), az1 = az0 + kPrimeZ;
    const uint32_t m = d.last;
    t[0] = ((ay0 ^ az0) & m) / (uint32_t)kTileEntries; t[1] = ((ay1 ^ az0) & m) / (uint32_t)kTileEntries;
    t[2] = ((ay0 ^ az1) & m) / (uint32_t)kTileEntries; t[3] = ((ay1 ^ az1) & m) / (uint32_t)kTileEntries;
}
// dense level: byte = tile of the x0 corner, bit 7 set when the x1 corner sits in the next chunk (= next tile); 0x7f (no tile) when
// the pair would wrap past the end of the level (the owners apply such a sample corner by corner, see bwd_stream_codes).
// With i1 = i0 + 1: "i1 >= size or i1 == 0" is i0 >= size - 1, and the chunks of the two differ exactly when i0 is the last entry of
// its chunk -- then the tiles differ too, as there are at least two.
template <bool INSIDE>
__device__ __forceinline__ uint32_t dense_code(const CodeLevel& d, float x, float y, float z) {
    const uint32_t gy = code_cell<INSIDE>(y, d.scale), gz = code_cell<INSIDE>(z, d.scale), gx = code_cell<INSIDE>(x, d.scale);
    const uint32_t base = gx + gy * d.res + gz * d.res2;
    uint32_t code = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t i0 = base + ((c & 1) ? d.res : 0u) + ((c >> 1) ? d.res2 : 0u);
        uint32_t b = ((i0 / kChunk) & d.tmask) | ((((i0 % kChunk) + 1u) * (0x80u / kChunk)) & 0x80u);
        if (i0 >= d.last) b = 0x7fu;
        code |= b << (8 * c);
    }
    return code;
}
// The same four bytes at once, for cells in [0, 16383) of a kCodeDense level (no index wraps): corner c is base + off_c, so
//   its place in its chunk is  (base % 32 + off_c % 32) % 32          (the sum is at most 62: it stays in its byte),
//   its chunk, modulo 64, is   (base / 32 % 64 + off_c / 32 % 64 + carry of the sum above) % 64     (at most 127),
// and the tile is the chunk modulo the number of tiles, a power of two up to 64.  top: the largest x0 corner seen; when that has no x1
// corner in the level (top >= last) some byte may have to be 0x7f, and the caller takes dense_code.
__device__ __forceinline__ uint32_t byte4(uint32_t v) { return __builtin_amdgcn_perm(v, v, 0u); }      // the low byte of v in all four bytes (v * 0x01010101 is a quarter-rate multiply)
__device__ __forceinline__ uint32_t dense_code_packed(const CodeLevel& d, float x, float y, float z, uint32_t& top) {
    const uint32_t gy = code_cell<true>(y, d.scale), gz = code_cell<true>(z, d.scale), gx = code_cell<true>(x, d.scale);
    const uint32_t base = gx + __umul24(gy, d.res) + __umul24(gz, d.res2);
    top = max(top, base + d.res + d.res2);
    const uint32_t place = byte4(base % kChunk) + d.off5;
    const uint32_t next = (((place & 0x1f1f1f1fu) + 0x01010101u) << 2) & 0x80808080u;      // bit 7: the last entry of its chunk
    const uint32_t chunk = byte4((base / kChunk) & 63u) + d.offc + ((place >> 5) & 0x01010101u);
    return (chunk & d.tmask4) | next;
}

// One coded level of a lane's four consecutive samples (cnt >= 1 of them live): the codes, stored with one 16-byte store (cnt < 4:
// element by element) -- a bit-row level's four 16-bit masks are handed back in m01 / m23 instead (samples 0, 1 and 2, 3; zero for a
// sample past cnt), for store_bit_rows --; returns the level's escape bit.  The kind is branched on once, around the four samples.
// INSIDE: every grid position of the four samples is in [0, 16383) (or NaN) at this level.
template <bool INSIDE>
__device__ __forceinline__ uint32_t code_level(const CodeLevel& d, const float (&p)[12], int cnt, int64_t i0, uint32_t* __restrict__ codes,
                                               const float2* __restrict__ dfeat, int64_t n, uint32_t& m01, uint32_t& m23) {
    const uint32_t kind = d.kind_level & 0xffu;
    uint32_t code[4];
    if (kind == kCodeMasks) {           // 16-bit masks of the tiles the four combinations name
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t t[4];
            hashed_tiles<INSIDE>(d, p[3 * k + 1], p[3 * k + 2], t);
            code[k] = k < cnt ? (1u << t[0]) | (1u << t[1]) | (1u << t[2]) | (1u << t[3]) : 0u;
        }
        m01 = code[0] | (code[1] << 16);
        m23 = code[2] | (code[3] << 16);
    } else {                            // one byte per combination
        if (kind == kCodeBytes) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t t[4];
                hashed_tiles<INSIDE>(d, p[3 * k + 1], p[3 * k + 2], t);
                code[k] = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
            }
        } else {
            uint32_t top = 0xffffffffu;
            if (INSIDE && kind == kCodeDense) {
                top = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) code[k] = dense_code_packed(d, p[3 * k], p[3 * k + 1], p[3 * k + 2], top);
            }
            if (top >= d.last) {
#pragma unroll
                for (int k = 0; k < 4; ++k) code[k] = dense_code<INSIDE>(d, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
            }
        }
        uint32_t* row = codes + d.row + i0;
        if (cnt == 4) {
            *reinterpret_cast<uint4*>(row) = make_uint4(code[0], code[1], code[2], code[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) row[k] = code[k];
        }
    }
    uint32_t esc = 0u;
    if (!INSIDE && (kind == kCodeMasks || kind == kCodeBytes)) {
        // a position so far outside the unit cube that its x-corners leave the first 16384 columns breaks "(y,z) decides the tile":
        // harmless without gradient; with gradient the level's owners take the generic path
        const uint32_t l = d.kind_level >> 8;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt && code_cell<false>(p[3 * k], d.scale) >= (uint32_t)(kTileEntries - 1)) {
                const float2 g = dfeat[(int64_t)l * n + i0 + k];
                if (!(g.x == 0.f && g.y == 0.f)) esc = 1u << l;
            }
    }
    return esc;
}

// The bit rows of one level from the masks of a wave's 256 samples (m01 / m23 of code_level; zero on lanes without live samples).  Per
// DPP row of 16 lanes and per sample slot the masks are a 16 x 16 bit matrix, lane by tile, two slots to a register; four butterfly
// stages (partner = lane ^ 8, 4, 2, 1: the halves of a block of bits change places between the two lanes) transpose it, so that lane t
// of the row ends with the bits of tile t: its 16 lanes' slot k in halfword k -- the bit order of bit_row_first_sample --, 8 bytes
// of the row's piece.  A stage is a lane exchange, a rotate and a bit select on each register: the rotate stands for the
// shift (left on the lower lane of a pair, right on the upper), as the bits it wraps around fall outside the half that is taken.
// Must be called by the whole wave.
template <int S>
__device__ __forceinline__ uint32_t bit_row_partner(uint32_t v) {
    if (S == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);        // row_ror:8
    if (S == 4) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101f);                           // lane ^ 4 (no LDS is touched)
    if (S == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, true);         // quad_perm:[2,3,0,1]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, true);                     // quad_perm:[1,0,3,2]
}
template <int S>
__device__ __forceinline__ uint32_t bit_row_stage(uint32_t v, uint32_t lane) {
    constexpr uint32_t kLow = S == 8 ? 0x00ff00ffu : (S == 4 ? 0x0f0f0f0fu : (S == 2 ? 0x33333333u : 0x55555555u));   // bits whose place has S clear
    const bool upper = (lane & (uint32_t)S) != 0u;
    const uint32_t keep = upper ? ~kLow : kLow;
    const uint32_t other = bit_row_partner<S>(v);
    const uint32_t moved = __builtin_amdgcn_alignbit(other, other, upper ? (uint32_t)S : 32u - (uint32_t)S);
    return (v & keep) | (moved & ~keep);
}
__device__ __forceinline__ void store_bit_rows(const CodeLevel& d, uint32_t m01, uint32_t m23, unsigned bx, uint32_t lane,
                                               uint32_t* __restrict__ codes, int64_t row_words) {
    m01 = bit_row_stage<8>(m01, lane); m23 = bit_row_stage<8>(m23, lane);
    m01 = bit_row_stage<4>(m01, lane); m23 = bit_row_stage<4>(m23, lane);
    m01 = bit_row_stage<2>(m01, lane); m23 = bit_row_stage<2>(m23, lane);
    m01 = bit_row_stage<1>(m01, lane); m23 = bit_row_stage<1>(m23, lane);
    // lane 16 r + t holds piece r of row t; lane 4 t + r stores it, so that the four lanes next to each other write a row's 32 bytes
    const uint32_t from = (((lane & 3u) << 4) | (lane >> 2)) << 2;
    m01 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)from, (int)m01);
    m23 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)from, (int)m23);
    const uint32_t t = lane >> 2;       // (rows above the level's tile count stay unwritten: nobody reads them)
    if (t <= d.tmask)
        *reinterpret_cast<uint2*>(codes + d.row + (int64_t)t * row_words + (int64_t)bx * (kCodeSamplesPerBlock / 32) + 2u * (lane & 3u)) = make_uint2(m01, m23);
}

// The tile codes of every coded level.  One workgroup = the 256 samples of one escape word: each of its four waves holds all 256 (four
// consecutive samples per lane: 48 bytes of positions in three 16-byte loads, one 16- or 8-byte store per level -- a bit-row level's
// after the wave has transposed its masks, store_bit_rows, outside the branches that lanes take apart --) and computes every
// fourth level, so that 1 M samples give a SIMD sixteen short waves, and the 16-35 k live rows of the reference-faithful training
// step (1 M-row capacity; the count is on the device) still some hundred waves; workgroups past the live count only write their
// (zero) escape word.  What bounds the kernel is its vector arithmetic (profiles/tile_codes_prepass.json), so the work per
// (sample, level) is kept short:
//  * one test per level and lane, on the smallest and the largest coordinate of the lane's samples (the grid position is monotonic
//    in the coordinate), says that every position of the level lies in [0, 16383) -- then nothing escapes, the cells need no floor
//    and a dense level's four bytes are formed at once (dense_code_packed); lanes that fail it take the exact path, so the codes are
//    the same for any input;
//  * the hashed levels multiply with the full-rate 24-bit multiplier (hashed_tiles);
//  * the exact dense byte takes two comparisons per corner (dense_code).
// (The launch can carry the MLP backward's second stage in workgroups of its own behind the `own_blocks` that compute codes:
//  mlp_reduce_device.hpp; and, in its FIRST draw.n_blocks workgroups, stage A of the step riders -- the next batch's draw and lattice
//  tables, step_riders_device.hpp: dispatched first, they run beside the code workgroups.)
__global__ __launch_bounds__(64 * kCodeWaves) void tile_codes4_kernel(CodePlan cp, const float* __restrict__ x01,
                                                                       const float2* __restrict__ dfeat, uint32_t* __restrict__ codes,
                                                                       uint32_t* __restrict__ escape, int64_t n,
                                                                       const int64_t* __restrict__ n_dev, MlpReduceJob job, unsigned own_blocks,
                                                                       RiderDrawJob draw) {
    if (blockIdx.x < (unsigned)draw.n_blocks) { rider_draw_block(draw, (int)blockIdx.x); return; }
    const unsigned bx = blockIdx.x - (unsigned)draw.n_blocks;
    if (bx >= own_blocks) { mlp_reduce_block(job, (int)(bx - own_blocks)); return; }
    const int64_t n_live = live_count(n, n_dev);            // n: capacity = stride of dfeat
    __shared__ uint32_t esc_block;
    if (threadIdx.x == 0) esc_block = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i0 = (int64_t)bx * kCodeSamplesPerBlock + 4 * lane;
    uint32_t esc = 0u;                  // bit l: level l must take the generic owners
    if ((int64_t)bx * kCodeSamplesPerBlock < n_live) {      // (the whole workgroup; lanes past the live count carry empty masks through the levels)
        const int cnt = i0 >= n_live ? 0 : ((n_live - i0) < 4 ? (int)(n_live - i0) : 4);
        const int64_t row_words = bit_row_words(n);
        float p[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (cnt == 0) {
        } else if (cnt == 4 && (reinterpret_cast<uintptr_t>(x01) & 15) == 0) {
            const float4 a = reinterpret_cast<const float4*>(x01 + 3 * i0)[0], b = reinterpret_cast<const float4*>(x01 + 3 * i0)[1],
                         c = reinterpret_cast<const float4*>(x01 + 3 * i0)[2];
            p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
            p[8] = c.x; p[9] = c.y; p[10] = c.z; p[11] = c.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = i0 + (k < cnt ? k : cnt - 1);
                p[3 * k] = x01[3 * i]; p[3 * k + 1] = x01[3 * i + 1]; p[3 * k + 2] = x01[3 * i + 2];
            }
        }
        float lo = p[0], hi = p[0];     // (fminf / fmaxf skip NaNs: a NaN coordinate's cell is 0 on either path; all NaN fails the test)
#pragma unroll
        for (int k = 1; k < 12; ++k) { lo = fminf(lo, p[k]); hi = fmaxf(hi, p[k]); }
        CodeLevel next = cp.lv[wave];
        for (int j = wave; j < cp.n_coded; j += kCodeWaves) {
            const CodeLevel d = next;
            next = cp.lv[j + kCodeWaves];
            uint32_t m01 = 0u, m23 = 0u;
            if (cnt == 0) {
            } else if (grid_pos(lo, d.scale) >= 0.f && grid_pos(hi, d.scale) < (float)(kTileEntries - 1))
                esc |= code_level<true>(d, p, cnt, i0, codes, dfeat, n, m01, m23);
            else
                esc |= code_level<false>(d, p, cnt, i0, codes, dfeat, n, m01, m23);
            if ((d.kind_level & 0xffu) == kCodeMasks) store_bit_rows(d, m01, m23, bx, (uint32_t)lane, codes, row_words);
        }
    }
    if (esc) atomicOr(&esc_block, esc);
    __syncthreads();
    if (threadIdx.x == 0) escape[bx] = esc_block;       // every word is written: no zero-fill needed
}

// ---- levels of 256..2048 tiles (log2_hashmap_size 22..25): per-tile bitmaps ---------------------------------------
// Beyond 255 tiles a level used to fall back to global atomics (2.1e10/s: 6.6 ms per 1 M samples at L = 20, T = 2^22): that many
// owners cannot each TEST every sample.  They do not have to: the pre-pass leaves one BIT per (tile, sample) -- row (level,
// tile) has bit i set when a (y,z) combination of sample i falls in the tile -- and an owner reads only its own row,
// 128 KiB per million samples, of which 4/tiles of the bits are set.  Rows are staged in LDS per block of 256 samples
// (tiles x 32 bytes) and written out whole, so the bitmaps need no zero fill; an owner gathers position and gradient of
// its few thousand samples lane by lane and works out the combinations from the (y,z) it gathered.  The cost of a level is
// its bitmap traffic (tiles x n / 8 bytes written and read once) plus 128 KiB of LDS zeroing and write-back per owner.
__global__ __launch_bounds__(256) void tile_bitmap_kernel(GridParams gp, TileParams tp, const float* __restrict__ x01,
                                                          const float2* __restrict__ dfeat, uint32_t* __restrict__ bitmaps,
                                                          uint32_t* __restrict__ esc_bm, int64_t n, const int64_t* __restrict__ n_dev) {
    const int64_t n_live = live_count(n, n_dev);
    int l = 0;
    while (!((tp.bitmap_levels >> l) & 1u) || tp.bm_idx[l] != (int)blockIdx.y) ++l;
    const int nt = tp.tiles_of[l];
    const int seg = tp.bm_samples / 32;         // words of a row this block writes (a block takes bm_samples samples: the larger,
                                                // the longer the contiguous pieces of the rows -- 128 bytes at 1024)
    extern __shared__ uint32_t stage[];         // [tile][seg]: the block's bits of every row
    __shared__ uint32_t esc_block;
    for (int r = threadIdx.x; r < nt * seg; r += 256) stage[r] = 0u;
    if (threadIdx.x == 0) esc_block = 0u;
    __syncthreads();
    for (int local = threadIdx.x; local < tp.bm_samples; local += 256) {
        const int64_t i = (int64_t)blockIdx.x * tp.bm_samples + local;
        if (i >= n_live) break;
        const float x = x01[3 * i], y = x01[3 * i + 1], z = x01[3 * i + 2];
        const uint32_t gy = (uint32_t)(int32_t)floorf(grid_pos(y, gp.scale[l])), gz = (uint32_t)(int32_t)floorf(grid_pos(z, gp.scale[l]));
        const uint32_t gx = (uint32_t)(int32_t)floorf(grid_pos(x, gp.scale[l]));
        const uint32_t word = (uint32_t)local >> 5, bit = 1u << ((uint32_t)local & 31u);
        const uint32_t useg = (uint32_t)seg;
        bool bad;
        if (gp.hashed[l]) {
            const uint32_t ay0 = gy * kPrimeY, ay1 = ay0 + kPrimeY, az0 = gz * kPrimeZ, az1 = az0 + kPrimeZ;
            const uint32_t m = gp.size[l] - 1u;
            atomicOr(&stage[(((ay0 ^ az0) & m) / (uint32_t)kTileEntries) * useg + word], bit);
            atomicOr(&stage[(((ay1 ^ az0) & m) / (uint32_t)kTileEntries) * useg + word], bit);
            atomicOr(&stage[(((ay0 ^ az1) & m) / (uint32_t)kTileEntries) * useg + word], bit);
            atomicOr(&stage[(((ay1 ^ az1) & m) / (uint32_t)kTileEntries) * useg + word], bit);
            bad = gx >= (uint32_t)(kTileEntries - 1);       // "(y,z) decides the tile" does not hold (see tile_codes4_kernel)
        } else {            // dense: chunk-interleaved ownership; every corner on its own, indices past the end wrap (bwd_apply's rule),
                            // so these levels never escape
            const uint32_t res = gp.res[l], r2 = res * res, tmask = (uint32_t)nt - 1u;
            bad = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t idx = (gx + (uint32_t)(k & 1)) + (gy + (uint32_t)((k >> 1) & 1)) * res + (gz + (uint32_t)(k >> 2)) * r2;
                if (idx >= gp.size[l]) idx = idx % gp.size[l];
                atomicOr(&stage[((idx / kChunk) & tmask) * useg + word], bit);
            }
        }
        if (bad) {          // with gradient the level's owners take the generic path
            const float2 g = dfeat[(int64_t)l * n + i];
            if (!(g.x == 0.f && g.y == 0.f)) atomicOr(&esc_block, 1u);
        }
    }
    __syncthreads();
    uint32_t* rows = bitmaps + (int64_t)tp.bm_row[l] * tp.bm_row_words + (int64_t)blockIdx.x * seg;
    for (int r = threadIdx.x; r < nt * seg; r += 256) rows[(int64_t)(r / seg) * tp.bm_row_words + (r % seg)] = stage[r];
    if (threadIdx.x == 0) esc_bm[(int64_t)blockIdx.y * tp.bm_blocks + blockIdx.x] = esc_block;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// position of a lane among the set bits of a ballot
__device__ __forceinline__ uint32_t ballot_rank(unsigned long long b) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}
// One sample slot into the wave's queue: the lanes that hit append their entries in lane order.  (`queue` and `qn` are wave-uniform and
// live on the scalar unit -- the kernel takes the wave's number through readfirstlane --, so the address of a write is ONE vector
// instruction on the lane's rank: rank * 4 + scalar.)
__device__ __forceinline__ void enqueue1(uint32_t* queue, uint32_t& qn, bool hit, uint32_t e) {
    const unsigned long long b = __ballot(hit);
    if (b) {
        if (hit) (queue + qn)[ballot_rank(b)] = e;
        qn += (uint32_t)__popcll(b);
    }
}
// grid_pos and a difference as single instructions the compiler cannot pair with their neighbours.  Left to itself it works on two of
// a gathered sample's three coordinates with two-wide f32 instructions (v_pk_fma_f32, v_pk_add_f32: y and z arrive as a register
// pair; with z taken out it pairs y with x), each of which holds a wave's issue about three times as long as the two plain
// instructions it stands for.  The same instructions on the same operands: the same bits.
__device__ __forceinline__ float grid_pos_alone(float x, float scale) {
    float r;
    asm("v_fma_f32 %0, %1, %2, 0.5" : "=v"(r) : "v"(x), "v"(scale));
    return r;
}
__device__ __forceinline__ float sub_alone(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// byte offsets of sample i's gradient (8 i) and position (12 i) by shifts and adds: i may exceed 2^24 (no 24-bit multiply), and
// the 32-bit multiply is quarter rate.  (The empty asm keeps the two shifts from being folded back into i * 12.)
__device__ __forceinline__ void sample_offsets(uint32_t i, uint32_t& ox, uint32_t& og) {
    og = i << 3;
    asm("" : "+v"(og));
    ox = (i << 2) + og;
}

// The loads of this loop are issued through inline assembly with hand-placed s_waitcnt: the compiler's own
// placement waits for a gather right where it is issued (it packs the loaded y,z into a register pair for a packed
// multiply) and drains vmcnt to 0 around the conditional drain.  VMEM loads return in issue order, so
// "vmcnt(k)" = "everything but the k youngest loads has landed"; the number of loads issued per step is static
// (2 code loads, then 2 gather loads per drain, idle lanes gather sample 0).  A sample's position is ONE 12-byte load
// (global_load_dwordx3; 4-byte alignment is all it asks): as a 4-byte and an 8-byte load of the same line the address unit walked the
// 64 lanes twice, and that walk, not arithmetic, is what the owners of the fine levels wait for in a training step -- their queued
// samples are scattered, a line per lane (302 -> 281 us per workgroup at the finest levels, the coarse ones unchanged).
// (Round 4 also built 16-bit nibble codes -- two samples tested with four bit-parallel operations --: bit-identical, owners 378.9
//  vs 361.7 us per 1 M samples, profiles/r04_bwd_code16_ab.json; the variant is tools/exp/r05_retired_variants.diff.)
template <bool FIXED, bool DENSE>
__device__ __forceinline__ void bwd_stream_codes(const BwdCtx& cx, float* lds_tile, uint32_t* queue,
                                                 const uint32_t* __restrict__ codes_l, const float* __restrict__ x01,
                                                 const float2* __restrict__ g_l, int64_t n, int rep, int R) {
    // (tells the compiler's own wait-count bookkeeping that nothing it knows of is in flight when the loop starts;
    //  otherwise it drains vmcnt to 0 at the head of every iteration on behalf of the other streaming variants)
    __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0)
    constexpr int kPer = 4;                             // samples of a lane per iteration (= per pair of code loads)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qn = 0;                                    // wave-uniform queue fill
    const int64_t n_full = n / kPer;
    const int64_t g_lo = n_full * rep / R, g_hi = n_full * (rep + 1) / R;       // this replica's groups of kPer samples
    // registers written by loads in flight: only ever read behind the waits below
    f32x3 ld_p = {0.f, 0.f, 0.f}; f32x2 ld_g = {0.f, 0.f}; u32x2 ld_c0 = {0u, 0u}, ld_c1 = {0u, 0u};
    uint32_t bcm = 0, bi = 0;                           // (y,z) combinations and sample index of the batch in flight
    bool blive = false;                                 // this lane holds an entry of the batch in flight
    const uint32_t t_split = 0x80u | cx.t, t_next = 0x80u | ((cx.t - 1u) & (cx.n_tiles - 1u));     // dense codes
    // -> combinations that name this tile; dense: 0x10 when a combination of the sample wraps past the end of the level
    //    (byte 0x7f) -- such a sample is queued by EVERY owner of the level without combinations and applied corner by
    //    corner with bwd_apply's wrapping rule (a few per cent of random points, none of a scene that keeps clear of the
    //    upper faces of its box: no reason to hand the whole level to the generic owners)
    // Hashed levels: which of a code's four bytes name this tile, as 0x80 in each such byte -- x = code ^ (t in every byte) has a zero byte
    // there, and ~(((x & 0x7f..) + 0x7f..) | x | 0x7f..) marks zero bytes exactly (no carry leaves a byte).  Five vector instructions per
    // code (gfx950's three-input bit operation folds the AND and the NOR) where four byte compares, four selects and two ORs took eleven; the
    // four bits of the queue entry are made from the marks by ONE dot product with (1, 2, 4, 8), and only on the lanes that hit.
    // (t4: this tile in every byte; a lane without a group of its own in the last iteration compares against 0xff.., which is no tile of
    //  a hashed level -- at most 255 of them -- so that validity costs one select per iteration instead of one per code)
    const uint32_t t4 = cx.t * 0x01010101u;
    auto test_marks = [&](uint32_t code, uint32_t t4) {
        const uint32_t x = code ^ t4;
        const uint32_t a = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
        return ~(a | x | 0x7f7f7f7fu);
    };
    auto test = [&](uint32_t code) {
        uint32_t cm = 0;
        bool wraps = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t b = (code >> (8 * c)) & 0xffu;
            const bool hit = DENSE ? (b == cx.t || b == t_split || b == t_next) : (b == cx.t);
            cm |= (hit ? 1u : 0u) << c;
            if (DENSE) wraps = wraps || b == 0x7fu;
        }
        return wraps ? 0x10u : cm;
    };
    // queue entry of sample i: index << 4 | combinations (the index's low four bits are clear: the dot product's addend ORs them in)
    auto entry = [&](uint32_t cm, uint32_t i) { return (i << 4) | (cm & 15u); };
    auto entry_marks = [&](uint32_t marks, uint32_t i) {          // (hashed levels: `marks` of test_marks)
        return __builtin_amdgcn_udot4(marks >> 7, 0x08040201u, i << 4, false);
    };
    auto enqueue = [&](uint32_t cm, uint32_t i) { enqueue1(queue, qn, cm != 0u, entry(cm, i)); };
    auto enqueue_marks = [&](uint32_t marks, uint32_t i) { enqueue1(queue, qn, marks != 0u, entry_marks(marks, i)); };
    auto load_codes = [&](uint32_t grp) {               // 2 loads
        const uint32_t off = (grp < (uint32_t)g_hi ? grp : (uint32_t)g_hi - 1u) * 16u;
        asm volatile("global_load_dwordx2 %0, %2, %3\n\tglobal_load_dwordx2 %1, %2, %3 offset:8"
                     : "=&v"(ld_c0), "=&v"(ld_c1) : "v"(off), "s"(codes_l) : "memory");
    };
    auto pop_and_gather = [&]() {       // up to 64 queued samples: issue the 2 loads of their position and gradient
        // (readfirstlane: scalar min and subtract -- left to itself the compiler forms qn - take as a saturating VECTOR subtract)
        const uint32_t take = (uint32_t)__builtin_amdgcn_readfirstlane((int)(qn < 64u ? qn : 64u));
        __builtin_amdgcn_wave_barrier();
        uint32_t e = 0;
        if (lane < take) e = (queue + (qn - take))[lane];
        __builtin_amdgcn_wave_barrier();
        qn -= take;
        blive = lane < take;
        bcm = e & 15u;
        bi = e >> 4;
        uint32_t ox, og;
        sample_offsets(bi, ox, og);
        asm volatile("global_load_dwordx3 %0, %2, %3\n\tglobal_load_dwordx2 %1, %4, %5"
                     : "=&v"(ld_p), "=&v"(ld_g) : "v"(ox), "s"(x01), "v"(og), "s"(g_l) : "memory");
    };
    // wait until at most `younger` loads are in flight; the batch is then read from the registers it landed in (they are in-out
    // operands of the wait: the compiler must not move a read of them above it, and no copy is spent -- the batch is dead before the
    // next pop issues loads into them)
#define PERF_WAIT_BATCH(younger)                                                                                        \
    asm volatile("s_waitcnt vmcnt(" #younger ")" : "+v"(ld_p), "+v"(ld_g) : : "memory");                                \
    const float bx = ld_p.x; const f32x2 byz = {ld_p.y, ld_p.z}, bg = ld_g
    // The batch gathered one drain ago.  Every lane applies ONE combination (loop-free at full occupancy); the 7 % of
    // samples that name this tile with two or more combinations go back into the queue with the remaining ones.
    auto apply_batch = [&](float bx, f32x2 byz, f32x2 bg) {
        if (DENSE && blive && bcm == 0u) {      // a sample with a wrapping corner: every corner on its own
            if (!(bg.x == 0.f && bg.y == 0.f)) bwd_apply<FIXED, false>(cx, lds_tile, make_float2(bg.x, bg.y), bx, byz.x, byz.y);
            return;
        }
        const uint32_t rest = DENSE ? 0u : bcm & (bcm - 1u);        // (dense tiles are named by several combinations as a rule)
        if (!DENSE) bcm &= 0u - bcm;
        if (bcm) {
            const float px = grid_pos(bx, cx.scale), py = grid_pos_alone(byz.x, cx.scale), pz = grid_pos_alone(byz.y, cx.scale);
            const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
            const uint32_t gx = (uint32_t)(int32_t)flx, gy = (uint32_t)(int32_t)fly, gz = (uint32_t)(int32_t)flz;
            // (only the low 24 bits of the (y,z) terms count on a coded level -- kMaxCodedHashedTiles -- and those are the low 24 bits
            //  of the full-rate 24-bit product of the factors' low 24 bits, for any cell: hashed_tiles)
            if (DENSE)
                apply_pairs_dense<FIXED>(cx, lds_tile, make_float2(bg.x, bg.y), gx, px - flx, sub_alone(py, fly), sub_alone(pz, flz),
                                         __umul24(gy, cx.res), __umul24(gz, cx.r2), bcm);
            else if (gx < (uint32_t)(kTileEntries - 1))      // (else: zero gradient, see tile_codes4_kernel)
                apply_pair_one<FIXED>(cx, lds_tile, make_float2(bg.x, bg.y), gx, px - flx, sub_alone(py, fly), sub_alone(pz, flz),
                                      __umul24(gy, kPrimeY & 0xffffffu), __umul24(gz, kPrimeZ & 0xffffffu), bcm);
        }
        if (!DENSE) enqueue(rest, bi);
    };
    if (g_hi > g_lo) {
        // (groups and sample indices fit 32 bits: kMaxCodedSamples; the trip count is wave-uniform and kept on the scalar unit)
        const uint32_t g_end = (uint32_t)g_hi;
        uint32_t grp = (uint32_t)g_lo + threadIdx.x;
        load_codes(grp);
        pop_and_gather();               // empty queue: dummy gather, keeps the in-flight count of the loop static
        for (uint32_t base = (uint32_t)g_lo + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)); base < g_end; base += kBwdThreads) {
            u32x2 c0, c1;               // in flight, oldest first: 2 code loads, 2 gather loads
            asm volatile("s_waitcnt vmcnt(2)\n\tv_mov_b64 %0, %2\n\tv_mov_b64 %1, %3" : "=&v"(c0), "=&v"(c1) : "v"(ld_c0), "v"(ld_c1) : "memory");
            const uint32_t g0 = grp;
            const bool valid = g0 < g_end;
            grp += kBwdThreads;
            load_codes(grp);
            const uint32_t cs[4] = {c0.x, c0.y, c1.x, c1.y};
            const uint32_t t4v = valid ? t4 : 0xffffffffu;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (DENSE) enqueue(valid ? test(cs[s]) : 0u, 4u * g0 + (uint32_t)s);
                else enqueue_marks(test_marks(cs[s], t4v), 4u * g0 + (uint32_t)s);
            }
            {
                PERF_WAIT_BATCH(2);         // all but the 2 code loads
                apply_batch(bx, byz, bg);
            }
            pop_and_gather();
            while (qn >= 128u) {            // bursts (ray-coherent samples at coarse hashed levels)
                PERF_WAIT_BATCH(0);
                apply_batch(bx, byz, bg);
                pop_and_gather();
            }
        }
    }
    if (threadIdx.x < 64 && rep == 0) {                 // ragged tail (n % kPer samples)
        const int64_t i = n_full * kPer + lane;
        uint32_t cm = 0u;
        if (i < n) cm = DENSE ? test(codes_l[i]) : test_marks(codes_l[i], t4);
        if (DENSE) enqueue(cm, (uint32_t)i);
        else enqueue_marks(cm, (uint32_t)i);
    }
    for (;;) {
        PERF_WAIT_BATCH(0);
        apply_batch(bx, byz, bg);
        bcm = 0; blive = false;
        if (qn == 0u) break;
        pop_and_gather();
    }
    asm volatile("" : : "v"(ld_c0), "v"(ld_c1));       // (the last code loads landed with the vmcnt(0) above)
#undef PERF_WAIT_BATCH
}

// inclusive prefix sum over the 64 lanes of a wave (DPP: shifts inside rows of 16, then row broadcasts)
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);      // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);      // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);      // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);      // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2, 3
    return v;
}

// ---- hashed owners of a bit-row level (at most 16 tiles: kMaskTiles) ----------------------------------------------
// An owner reads ITS row only -- one bit per sample, n / 8 bytes -- and pays per hit instead of per sample: a lane takes one halfword
// of the row per round (16 samples; the wave 1,024: kBitRoundSamples), the wave places its hits with one popcount and one scan, and
// every lane appends its set bits to the wave's queue (about 225 of 1,024 at 16 tiles: 8-9 trips of the longest lane).  A fresh queue
// entry carries cm = 0, as the row does not say WHICH of the sample's four (y,z) combinations name the tile: the apply works them out
// from the (y,z) it gathered anyway, with the pre-pass's own four tile expressions (hashed_tiles); re-queued entries carry their
// remaining combinations.  The queue is drained 64 entries at a time while it holds that many, so the applies run at full lanes.
// TWO gather batches take turns (PERF_BITS_HALF): the queue is drained in bursts of three or four pops between two rounds, and with
// one batch every pop but the first of a burst was waited for right where it was issued.  The wait counts are static: a half waits
// until its own pop's 2 loads are the only ones in flight, a round is taken behind "vmcnt(0)", and the row's next halfword is
// requested at the end of the half that took a round.
// Queue bound (kQueueCap): the queue is fed when it holds fewer than 64 entries, with one batch waiting to be applied, which re-queues
// at most 64.  A round of at most kQueueCap - 64 - (entries held) hits is appended whole; a fuller one (a run of samples in one cell
// of a coarse level; any round of a level of 2 tiles) goes in by nibbles -- at most 4 x 64 hits each -- with drains between.
constexpr int kBitRoundSamples = 16 * 64;
static_assert(64 + kBitRoundSamples / 4 + 64 <= kQueueCap, "bwd_stream_bits: a nibble of a round and the apply's re-queue must fit the queue");
struct GatherBatch {
    f32x3 ld_p; f32x2 ld_g;             // written by loads in flight: only ever read behind the wait of PERF_BITS_HALF
    uint32_t cm, i;                     // combinations (0: not known yet) and sample index of the lane's entry
    bool live;                          // this lane holds an entry
};

template <bool FIXED>
__device__ __forceinline__ void bwd_stream_bits(const BwdCtx& cx, float* lds_tile, uint32_t* queue,
                                                const uint32_t* __restrict__ row, const float* __restrict__ x01,
                                                const float2* __restrict__ g_l, int64_t n, int rep, int R) {
    __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0), see bwd_stream_codes
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qn = 0;                                    // wave-uniform queue fill
    // halfwords of the row that hold live samples (the pre-pass writes a block's pieces whole), and this replica's share of them
    const int64_t h_all = (n + kCodeSamplesPerBlock - 1) / kCodeSamplesPerBlock * (kCodeSamplesPerBlock / 16);
    const int64_t h_lo = h_all * rep / R, h_hi = h_all * (rep + 1) / R;
    uint32_t ld_w = 0u;                                 // written by the load in flight
    GatherBatch A = {{0.f, 0.f, 0.f}, {0.f, 0.f}, 0u, 0u, false}, B = A;          // the two batches that take turns in flight
    const uint32_t t_hi = cx.t * (uint32_t)kTileEntries, m_hi = cx.mask & ~(uint32_t)(kTileEntries - 1);
    // (fresh entries: index << 4, the combinations not known yet; re-queued ones carry theirs)
    auto requeue = [&](uint32_t cm, uint32_t i) __attribute__((always_inline)) { enqueue1(queue, qn, cm != 0u, (i << 4) | cm); };
    auto load_row = [&](uint32_t h) __attribute__((always_inline)) {                   // 1 load
        const uint32_t off = (h < (uint32_t)h_hi ? h : (uint32_t)h_hi - 1u) * 2u;
        asm volatile("global_load_ushort %0, %1, %2" : "+v"(ld_w) : "v"(off), "s"(row) : "memory");      // (in-out: the one register on every path)
    };
    // the set bits of a lane's halfword as entries behind the wave's: bit b is sample s0 + 4 b (bit_row_first_sample), e0 = s0 << 4.
    // incl: the inclusive wave prefix of the popcounts; the caller made room.
    auto append = [&](uint32_t bits, uint32_t e0, uint32_t incl) __attribute__((always_inline)) {
        uint32_t* q = queue + qn + (incl - (uint32_t)__popc(bits));
        while (bits) {
            const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            *q++ = e0 + (b << 6);
        }
        qn += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    };
    // up to 64 queued samples into batch X: 2 loads; returns how many
    auto pop_and_gather = [&](GatherBatch& X) __attribute__((always_inline)) {
        // (readfirstlane: scalar min and subtract -- left to itself the compiler forms qn - take as a saturating VECTOR subtract)
        const uint32_t take = (uint32_t)__builtin_amdgcn_readfirstlane((int)(qn < 64u ? qn : 64u));
        __builtin_amdgcn_wave_barrier();
        uint32_t e = 0;
        if (lane < take) e = (queue + (qn - take))[lane];
        __builtin_amdgcn_wave_barrier();
        qn -= take;
        X.live = lane < take;
        X.cm = e & 15u;
        X.i = e >> 4;
        uint32_t ox, og;
        sample_offsets(X.i, ox, og);
        asm volatile("global_load_dwordx3 %0, %2, %3\n\tglobal_load_dwordx2 %1, %4, %5"
                     : "+v"(X.ld_p), "+v"(X.ld_g) : "v"(ox), "s"(x01), "v"(og), "s"(g_l) : "memory");     // (in-out: the batch's one register set)
        return take;
    };
    // Every lane applies ONE combination; the samples that name this tile with two or more go back into the queue with the rest.
    auto apply_batch = [&](const GatherBatch& X, float bx, f32x2 byz, f32x2 bg) __attribute__((always_inline)) {
        const float px = grid_pos(bx, cx.scale), py = grid_pos_alone(byz.x, cx.scale), pz = grid_pos_alone(byz.y, cx.scale);
        const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
        const uint32_t gx = (uint32_t)(int32_t)flx;
        // (a bit-row level has at most 2^18 entries: only the low 24 bits of the (y,z) terms count, and those are the low 24 bits of
        //  the full-rate 24-bit product of the factors' low 24 bits, for any cell -- the pre-pass's own expressions, hashed_tiles)
        const uint32_t ay0 = __umul24((uint32_t)(int32_t)fly, kPrimeY & 0xffffffu), az0 = __umul24((uint32_t)(int32_t)flz, kPrimeZ & 0xffffffu);
        const uint32_t ay1 = ay0 + kPrimeY, az1 = az0 + kPrimeZ;
        // (tile == t, with the tile's bits of the index compared in place)
        const uint32_t derived = ((((ay0 ^ az0) & m_hi) == t_hi) ? 1u : 0u) | ((((ay1 ^ az0) & m_hi) == t_hi) ? 2u : 0u) |
                                 ((((ay0 ^ az1) & m_hi) == t_hi) ? 4u : 0u) | ((((ay1 ^ az1) & m_hi) == t_hi) ? 8u : 0u);
        uint32_t cm = X.cm ? X.cm : derived;
        if (!X.live || gx >= (uint32_t)(kTileEntries - 1)) cm = 0u;     // (idle lane; or zero gradient, see tile_codes4_kernel)
        const uint32_t rest = cm & (cm - 1u);
        cm &= 0u - cm;
        if (cm) apply_pair_one<FIXED>(cx, lds_tile, make_float2(bg.x, bg.y), gx, px - flx, sub_alone(py, fly), sub_alone(pz, flz), ay0, az0, cm);
        requeue(rest, X.i);
    };
    // One half of the loop's body: feed the queue when it runs low, pop batch Y, then wait for batch X -- popped one half earlier --
    // and apply it from the registers it landed in.  Each batch has ONE pop and ONE apply in the text of the loop, and its registers
    // are in-out operands of both: wherever a pop or an apply stood twice, the compiler gave the batch a register set per place and
    // copied between them while its loads were in flight (a wait count chosen by a branch between two such statements did the same).
    // In flight at the wait, oldest first: [X: 2][the row][Y: 2], or the batches alone, so the wait leaves 2 loads out.
    // (After a change to this loop, compare the registers of the loads with those of the waits and the applies in the assembly.)
#define PERF_BITS_HALF(X, Y)                                                                                            \
    {                                                                                                                   \
        const bool fed = feed();                                                                                        \
        const uint32_t popped = pop_and_gather(Y);                                                                      \
        asm volatile("s_waitcnt vmcnt(2)" : "+v"(X.ld_p), "+v"(X.ld_g) : : "memory");                                   \
        apply_batch(X, X.ld_p.x, f32x2{X.ld_p.y, X.ld_p.z}, X.ld_g);                                                    \
        if (fed && base < h_end) load_row(h);                                                                           \
        if (popped == 0u && qn == 0u && nibble == 4 && base >= h_end) break;                                            \
    }
    const uint32_t h_end = (uint32_t)h_hi;              // (halfwords and sample indices fit 32 bits: kMaxCodedSamples)
    uint32_t h = (uint32_t)h_lo + threadIdx.x;
    // the round to take next, wave-uniform and kept on the scalar unit
    uint32_t base = (uint32_t)h_lo + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    uint32_t rest = 0u, e0 = 0u;        // what is left of a round that did not fit, and its lanes' first entries
    int nibble = 4;                     // the next nibble of `rest` (4: none left)
    // the next round, or the next nibble of one that did not fit, once the queue holds fewer than 64 entries; true: a round was taken
    auto feed = [&]() __attribute__((always_inline)) {
        bool fed = false;
        if (qn < 64u && (nibble < 4 || base < h_end)) {
            if (nibble == 4) {
                uint32_t w;         // (the row may be the youngest load in flight)
                asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, %1" : "=&v"(w) : "v"(ld_w) : "memory");
                const uint32_t bits = h < h_end ? w : 0u;       // a lane without a halfword of its own in the last round hits nothing
                e0 = bit_row_first_sample(h) << 4;
                h += kBwdThreads;
                base += kBwdThreads;
                fed = true;
                const uint32_t incl = wave_inclusive_sum((uint32_t)__popc(bits));
                const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                if (qn + total <= (uint32_t)(kQueueCap - 64)) append(bits, e0, incl);
                else { rest = bits; nibble = 0; }
            }
            if (nibble < 4) {
                const uint32_t nib = rest & (0xfu << (4 * nibble));
                append(nib, e0, wave_inclusive_sum((uint32_t)__popc(nib)));
                ++nibble;
            }
        }
        return fed;
    };
    if (base < h_end) {
        load_row(h);
        (void)pop_and_gather(A);        // empty queue: dummy gather, keeps the in-flight count of the loop static
        for (;;) {
            PERF_BITS_HALF(A, B)
            PERF_BITS_HALF(B, A)
        }
        // (the last pop took nothing: its dummy loads land before the registers are anybody else's)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(A.ld_p), "+v"(A.ld_g), "+v"(B.ld_p), "+v"(B.ld_g) : : "memory");
    }
#undef PERF_BITS_HALF
    asm volatile("" : : "v"(ld_w));                     // (the last row load landed with a vmcnt(0) above)
}

// Owner of one tile of a bitmap level.  A wave reads 64 words of the row per step (2048 samples), turns the set bits into
// sample indices in its LDS queue with ONE wave scan (a row holds 4-5 / tiles of the samples), and applies the queue 64
// entries at a time at full lane occupancy: position and gradient gathered, the combinations that fall in this tile
// worked out from the gathered (y,z).  (Lanes that walk their own bits one after the other instead -- the first version --
// pay one memory latency per round and as many rounds as the fullest lane has bits: 0.10 ms per owner at 256 hashed
// tiles, 1.66 ms at 64 dense tiles.)  A step that would overflow the queue -- dense rows -- is fed nibble by nibble.
template <bool FIXED, bool DENSE>
__device__ __forceinline__ void bwd_stream_bitmap(const BwdCtx& cx, float* lds_tile, uint32_t* queue, const uint32_t* __restrict__ row,
                                                  const float* __restrict__ x01, const float2* __restrict__ g_l, int64_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qn = 0;                                    // wave-uniform queue fill
    auto drain = [&]() {                                // the youngest min(qn, 64) entries
        const uint32_t take = qn < 64u ? qn : 64u;
        __builtin_amdgcn_wave_barrier();
        const bool live = lane < take;
        const uint32_t i = live ? queue[qn - take + lane] : 0u;
        __builtin_amdgcn_wave_barrier();
        qn -= take;
        const float2 g = g_l[i];
        const float x = x01[3 * (size_t)i], y = x01[3 * (size_t)i + 1], z = x01[3 * (size_t)i + 2];
        if (!live || (g.x == 0.f && g.y == 0.f)) return;
        if (DENSE) { bwd_apply<FIXED, false>(cx, lds_tile, g, x, y, z); return; }      // (tests the tile of each corner, wraps indices)
        const float px = grid_pos(x, cx.scale), py = grid_pos(y, cx.scale), pz = grid_pos(z, cx.scale);
        const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
        const uint32_t gx = (uint32_t)(int32_t)flx;
        if (gx >= (uint32_t)(kTileEntries - 1)) return;          // (zero gradient or the level escaped, see tile_bitmap_kernel)
        const uint32_t ay0 = (uint32_t)(int32_t)fly * kPrimeY, az0 = (uint32_t)(int32_t)flz * kPrimeZ;
        const uint32_t ay1 = ay0 + kPrimeY, az1 = az0 + kPrimeZ;
        const uint32_t cm = ((((ay0 ^ az0) & cx.mask) / (uint32_t)kTileEntries) == cx.t ? 1u : 0u) |
                            ((((ay1 ^ az0) & cx.mask) / (uint32_t)kTileEntries) == cx.t ? 2u : 0u) |
                            ((((ay0 ^ az1) & cx.mask) / (uint32_t)kTileEntries) == cx.t ? 4u : 0u) |
                            ((((ay1 ^ az1) & cx.mask) / (uint32_t)kTileEntries) == cx.t ? 8u : 0u);
        if (cm) apply_pairs<FIXED>(cx, lds_tile, g, gx, px - flx, py - fly, pz - flz, ay0, az0, cm);
    };
    auto enqueue = [&](uint32_t bits, uint32_t s0, uint32_t incl) {    // set bit b of `bits` = sample s0 + b; incl = inclusive wave
                                                                        // prefix of the popcounts; the caller made room
        const uint32_t cnt = (uint32_t)__popc(bits);
        uint32_t at = qn + incl - cnt;
        while (bits) {
            const int b = __ffs((int)bits) - 1;
            bits &= bits - 1u;
            queue[at++] = s0 + (uint32_t)b;
        }
        qn += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    };
    const int64_t n_words = (n + 31) / 32;
    const int64_t w_first = (int64_t)(threadIdx.x >> 6) * 64 + lane, w_step = (int64_t)(kBwdThreads / 64) * 64;
    uint32_t next = w_first < n_words ? row[w_first] : 0u;
    for (int64_t w = w_first; w - lane < n_words; w += w_step) {     // wave-uniform trip count
        const uint32_t bits = next;
        next = (w + w_step < n_words) ? row[w + w_step] : 0u;
        const uint32_t incl = wave_inclusive_sum((uint32_t)__popc(bits));
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (qn + total <= (uint32_t)kQueueCap) {
            enqueue(bits, (uint32_t)w * 32u, incl);
            while (qn >= 64u) drain();
        } else {            // (at most 256 new entries per nibble, fewer than 64 left over from the one before)
#pragma unroll 1
            for (int s = 0; s < 8; ++s) {
                const uint32_t nib = (bits >> (4 * s)) & 15u;
                enqueue(nib, (uint32_t)w * 32u + 4u * (uint32_t)s, wave_inclusive_sum((uint32_t)__popc(nib)));
                while (qn >= 64u) drain();
            }
        }
    }
    while (qn) drain();
}

// Single-tile dense levels (the coarsest ones: a cell is several sample spacings wide): a thread walks consecutive
// samples of a ray, so it sums a RUN of samples that share a cell in registers -- 8 packed corner sums -- and touches LDS
// only when the cell changes.  At res 16 / 23 that is a fifth / a quarter of the LDS atomics, which is what these
// owners were bound by (the lanes of a wave pile up on the few cells a scene populates).  Fixed point: same integers,
// same sums; fp32: a different (shorter) summation order.
template <bool FIXED>
struct RunAcc {
    uint32_t base;              // index of the run's (0,0,0) corner; 0xffffffff: empty
    long long v[8];             // FIXED: packed field pairs; else two floats bit-cast
};

template <bool FIXED>
__device__ __forceinline__ void run_flush(const BwdCtx& cx, float* lds_tile, RunAcc<FIXED>& r) {
    if (r.base == 0xffffffffu) return;
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds_tile);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t idx = r.base + (uint32_t)(k & 1) + ((k >> 1) & 1 ? cx.res : 0u) + ((k >> 2) ? cx.r2 : 0u);
        if (idx >= cx.size) idx = idx % cx.size;
        if (FIXED) {
            if (r.v[k] != 0ll) atomicAdd(&lds64[idx], (unsigned long long)r.v[k]);
        } else {
            const float a = __int_as_float((int)(uint32_t)(unsigned long long)r.v[k]), b = __int_as_float((int)(uint32_t)((unsigned long long)r.v[k] >> 32));
            unsafeAtomicAdd(&lds_tile[2 * idx], a); unsafeAtomicAdd(&lds_tile[2 * idx + 1], b);
        }
    }
}

template <bool FIXED>
__device__ __forceinline__ void run_apply(const BwdCtx& cx, float* lds_tile, RunAcc<FIXED>& r, const float2 g, const float x,
                                          const float y, const float z) {
    const float px = grid_pos(x, cx.scale), py = grid_pos(y, cx.scale), pz = grid_pos(z, cx.scale);
    const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
    float fx = px - flx, fy = py - fly, fz = pz - flz;
    const uint32_t base = (uint32_t)(int32_t)flx + (uint32_t)(int32_t)fly * cx.res + (uint32_t)(int32_t)flz * cx.r2;
    if (cx.smooth) { fx = fx * fx * (3.0f - 2.0f * fx); fy = fy * fy * (3.0f - 2.0f * fy); fz = fz * fz * (3.0f - 2.0f * fz); }
    const bool fresh = base != r.base;
    if (fresh) { run_flush<FIXED>(cx, lds_tile, r); r.base = base; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int bx = k & 1, by = (k >> 1) & 1, bz = k >> 2;
        const float w = ((bx ? fx : 1.0f - fx) * (by ? fy : 1.0f - fy)) * (bz ? fz : 1.0f - fz);        // association of bwd_apply
        if (FIXED) {
            const long long lo = (long long)__float2int_rn(w * g.x * cx.to_fixed);
            const long long hi = (long long)__float2int_rn(w * g.y * cx.to_fixed);
            const long long v = (hi << 32) + lo;
            r.v[k] = fresh ? v : r.v[k] + v;
        } else {
            const float a = w * g.x, b = w * g.y;
            const float pa = fresh ? 0.f : __int_as_float((int)(uint32_t)(unsigned long long)r.v[k]);
            const float pb = fresh ? 0.f : __int_as_float((int)(uint32_t)((unsigned long long)r.v[k] >> 32));
            r.v[k] = (long long)(((unsigned long long)(uint32_t)__float_as_int(pb + b) << 32) | (unsigned long long)(uint32_t)__float_as_int(pa + a));
        }
    }
}

// Streaming loop: a thread owns 4 consecutive samples per iteration -- 3 x 16 B of positions + 2 x 16 B of
// gradients, all 16-byte loads -- and the next group is in flight while the current one is applied.
template <bool FIXED, bool HASHED>
__device__ __forceinline__ void bwd_stream(const BwdCtx& cx, float* lds_tile, const float* __restrict__ x01,
                                           const float2* __restrict__ g_l, int64_t n, int rep, int R, const bool run_merge = false) {
    constexpr int kGroup = 4;
    const int64_t n_full = n / kGroup;
    const float4* x4 = reinterpret_cast<const float4*>(x01);
    const float4* g4 = reinterpret_cast<const float4*>(g_l);
    const bool aligned = ((reinterpret_cast<uintptr_t>(x01) | reinterpret_cast<uintptr_t>(g_l)) & 15) == 0;
    if (aligned && !HASHED) {
        // Dense levels: samples that follow each other along a ray fall into the same cell, i.e. the lanes of a wave
        // would all add to the same 8 LDS addresses (measured: ~70 cycles per ds_add instruction).  Each thread
        // therefore walks its OWN contiguous run of groups, starting at a lane-dependent rotation, so that the lanes
        // of a wave sit on different rays at different depths.
        const int64_t g_lo = n_full * rep / R, g_hi = n_full * (rep + 1) / R;
        const int64_t len = (g_hi - g_lo + kBwdThreads - 1) / kBwdThreads;
        const int64_t t_lo = g_lo + (int64_t)threadIdx.x * len;
        const int64_t mine = (t_lo >= g_hi) ? 0 : ((g_hi - t_lo < len) ? g_hi - t_lo : len);
        int64_t j = (len * (int64_t)(threadIdx.x & 63u)) / 64;        // rotation (wraps inside [0, len))
        float4 xa = {}, xb = {}, xc = {}, ga = {}, gb = {};
        auto fetch = [&](int64_t jj) {
            if (jj < mine) { const int64_t grp = t_lo + jj; xa = x4[3 * grp]; xb = x4[3 * grp + 1]; xc = x4[3 * grp + 2]; ga = g4[2 * grp]; gb = g4[2 * grp + 1]; }
        };
        fetch(j);
        if (run_merge && cx.n_tiles == 1u) {
            RunAcc<FIXED> run;
            run.base = 0xffffffffu;
            for (int64_t it = 0; it < len; ++it) {
                const float4 cxa = xa, cxb = xb, cxc = xc, cga = ga, cgb = gb;
                const bool live = j < mine;
                j = (j + 1 == len) ? 0 : j + 1;
                if (it + 1 < len) fetch(j);
                if (live) {
                    if (!(cga.x == 0.f && cga.y == 0.f)) run_apply<FIXED>(cx, lds_tile, run, make_float2(cga.x, cga.y), cxa.x, cxa.y, cxa.z);
                    if (!(cga.z == 0.f && cga.w == 0.f)) run_apply<FIXED>(cx, lds_tile, run, make_float2(cga.z, cga.w), cxa.w, cxb.x, cxb.y);
                    if (!(cgb.x == 0.f && cgb.y == 0.f)) run_apply<FIXED>(cx, lds_tile, run, make_float2(cgb.x, cgb.y), cxb.z, cxb.w, cxc.x);
                    if (!(cgb.z == 0.f && cgb.w == 0.f)) run_apply<FIXED>(cx, lds_tile, run, make_float2(cgb.z, cgb.w), cxc.y, cxc.z, cxc.w);
                }
            }
            run_flush<FIXED>(cx, lds_tile, run);
        } else
        for (int64_t it = 0; it < len; ++it) {
            const float4 cxa = xa, cxb = xb, cxc = xc, cga = ga, cgb = gb;
            const bool live = j < mine;
            j = (j + 1 == len) ? 0 : j + 1;
            if (it + 1 < len) fetch(j);
            if (live) {
                if (!(cga.x == 0.f && cga.y == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cga.x, cga.y), cxa.x, cxa.y, cxa.z);
                if (!(cga.z == 0.f && cga.w == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cga.z, cga.w), cxa.w, cxb.x, cxb.y);
                if (!(cgb.x == 0.f && cgb.y == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cgb.x, cgb.y), cxb.z, cxb.w, cxc.x);
                if (!(cgb.z == 0.f && cgb.w == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cgb.z, cgb.w), cxc.y, cxc.z, cxc.w);
            }
        }
    } else if (aligned) {
        int64_t grp = (int64_t)rep * kBwdThreads + threadIdx.x;
        const int64_t gstride = (int64_t)R * kBwdThreads;
        float4 xa = {}, xb = {}, xc = {}, ga = {}, gb = {};
        if (grp < n_full) { xa = x4[3 * grp]; xb = x4[3 * grp + 1]; xc = x4[3 * grp + 2]; ga = g4[2 * grp]; gb = g4[2 * grp + 1]; }
        while (grp < n_full) {
            const float4 cxa = xa, cxb = xb, cxc = xc, cga = ga, cgb = gb;
            grp += gstride;
            if (grp < n_full) { xa = x4[3 * grp]; xb = x4[3 * grp + 1]; xc = x4[3 * grp + 2]; ga = g4[2 * grp]; gb = g4[2 * grp + 1]; }
            if (!(cga.x == 0.f && cga.y == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cga.x, cga.y), cxa.x, cxa.y, cxa.z);
            if (!(cga.z == 0.f && cga.w == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cga.z, cga.w), cxa.w, cxb.x, cxb.y);
            if (!(cgb.x == 0.f && cgb.y == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cgb.x, cgb.y), cxb.z, cxb.w, cxc.x);
            if (!(cgb.z == 0.f && cgb.w == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, make_float2(cgb.z, cgb.w), cxc.y, cxc.z, cxc.w);
        }
    }
    if (aligned) {
        if (rep == 0) {     // ragged tail (n % 4 samples)
            const int64_t i = n_full * kGroup + threadIdx.x;
            if (i < n) { const float2 g = g_l[i]; if (!(g.x == 0.f && g.y == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, g, x01[3 * i], x01[3 * i + 1], x01[3 * i + 2]); }
        }
    } else {
        for (int64_t i = (int64_t)rep * kBwdThreads + threadIdx.x; i < n; i += (int64_t)R * kBwdThreads) {
            const float2 g = g_l[i];
            if (!(g.x == 0.f && g.y == 0.f)) bwd_apply<FIXED, HASHED>(cx, lds_tile, g, x01[3 * i], x01[3 * i + 1], x01[3 * i + 2]);
        }
    }
}

// FIXED = true: the two features of an entry are accumulated as two signed 32-bit fixed-point fields packed in one
// 64-bit LDS word (sum of h*2^32 + l is exact integer arithmetic; fields are recovered at write-back) with ONE
// full-rate integer ds_add_u64 per corner -- gfx950 serialises ds_add_f32 at ~3 cycles per active lane
// (tools/exp/lds_atomics.hip).  The unit is a power of two derived on the device from the level's max |dfeat|:
// unit = 2^ceil(log2(absmax)) * 2^(headroom - 31).  A tile whose largest field comes within 2x of the int32 range
// raises *overflow_flag (the caller then falls back to the fp32 mode).
template <bool FIXED>
__global__ __launch_bounds__(kBwdThreads) void hashgrid_bwd_kernel(GridParams gp, TileParams tp,
                                                                   const float* __restrict__ x01,
                                                                   const float2* __restrict__ dfeat,
                                                                   float2* __restrict__ grad, float2* __restrict__ ws,
                                                                   const float* __restrict__ level_absmax,
                                                                   int32_t* __restrict__ overflow_flag,
                                                                   int32_t* __restrict__ hr_state,
                                                                   const int32_t* __restrict__ shifts_in,
                                                                   int32_t* __restrict__ shifts_ws,
                                                                   const uint32_t* __restrict__ codes,
                                                                   const uint32_t* __restrict__ escape,
                                                                   const uint32_t* __restrict__ bitmaps,
                                                                   const uint32_t* __restrict__ esc_bm, int64_t n,
                                                                   const int64_t* __restrict__ n_dev,
                                                                   const int32_t* __restrict__ redo_flag, perf_step_book book, int has_book) {
    // a predicated REDO launch (perf_hashgrid_bwd, redo_flag): nothing happens unless the fixed-point call before it raised
    // the flag -- the graph node costs a dispatch, the gradient table is left as that call wrote it.  The dispatch exists in every
    // training step: ONE of its threads does the step's bookkeeping on the way (perf_field_bwd_book) -- everything but clearing the
    // flag, which every workgroup of this launch reads right here (perf_adam_step_dev's clear_flag consumes it afterwards)
    if constexpr (!FIXED) {
        if (redo_flag && has_book && blockIdx.x == 0 && threadIdx.x == 0) step_bookkeeping_thread(book, false);
    }
    if (redo_flag && redo_flag[0] == 0) return;
    if (redo_flag && hr_state && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&hr_state[2 * PERF_MAX_LEVELS + 1], 1);   // (statistics)
    const int64_t n_live = live_count(n, n_dev);            // samples present; n stays the stride of dfeat / codes
    extern __shared__ __attribute__((aligned(16))) float lds_tile[];   // 2 * kTileEntries floats (+ the wave queues)
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds_tile);
    int b = blockIdx.x, l = 0;
    uint32_t t;
    int rep;
    if (tp.use_work) {
        const uint32_t wk = tp.work[blockIdx.x];
        if (wk == 0xffffffffu) return;
        l = (int)(wk >> 16); t = (wk >> 8) & 0xffu; rep = (int)(wk & 0xffu);
    } else {
        while (b >= tp.tiles_of[l] * tp.replicas_of[l]) { b -= tp.tiles_of[l] * tp.replicas_of[l]; ++l; }
        t = (uint32_t)(b / tp.replicas_of[l]);
        rep = b % tp.replicas_of[l];
    }
    const int R = tp.replicas_of[l];
    const uint32_t n_tiles = (uint32_t)tp.tiles_of[l];
    const uint32_t size = gp.size[l];
    const bool hashed = gp.hashed[l] != 0;
#ifdef PERF_BWD_BLOCK_TIMES         // tools/exp/bwd_block_times.py: the launch is as long as its SLOWEST workgroup -- which one is it?
    const long long block_t0 = wall_clock64();
#endif
    for (int i = threadIdx.x; i < 2 * kTileEntries / 4; i += kBwdThreads)
        reinterpret_cast<float4*>(lds_tile)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    float from_fixed = 1.0f;
    BwdCtx cx;
    cx.scale = gp.scale[l]; cx.res = gp.res[l]; cx.r2 = cx.res * cx.res; cx.size = size; cx.mask = size - 1u;
    cx.n_tiles = n_tiles; cx.t = t; cx.tile_shift = (uint32_t)(__ffs((int)n_tiles) - 1);
    cx.smooth = gp.interpolation == PERF_INTERP_SMOOTHSTEP;
    cx.to_fixed = 1.0f;
    if (FIXED) {
        // units per 1.0 = 2^sh: given by the caller (job-wide units of a data-parallel step) or derived here; the level's
        // first workgroup leaves it for the replica reduction
        const int sh = shifts_in ? shifts_in[l] : fixed_point_shift(level_absmax[l], n_live, size, hr_state, l);
        cx.to_fixed = ldexpf(1.0f, sh);
        from_fixed = ldexpf(1.0f, -sh);
        if (shifts_ws && t == 0u && rep == 0 && threadIdx.x == 0) shifts_ws[l] = sh;
    }
    const float2* g_l = dfeat + (int64_t)l * n;
    bool coded = codes && tp.code_slot[l] >= 0;
    if (coded) {                        // any escape bit for this level in the pre-pass blocks' words?
        __shared__ uint32_t esc_any;
        if (threadIdx.x == 0) esc_any = 0u;
        __syncthreads();
        uint32_t e = 0u;
        const int64_t n_words = (n_live + kCodeSamplesPerBlock - 1) / kCodeSamplesPerBlock;      // (blocks without live samples wrote 0)
        for (int64_t w = threadIdx.x; w < n_words; w += kBwdThreads) e |= escape[w];
        if ((e >> l) & 1u) esc_any = 1u;
        __syncthreads();
        coded = esc_any == 0u;
    }
    bool by_bitmap = bitmaps && ((tp.bitmap_levels >> l) & 1u);
    if (by_bitmap) {                    // (same escape rule as the coded levels: one word per pre-pass block and level)
        __shared__ uint32_t esc_bm_any;
        if (threadIdx.x == 0) esc_bm_any = 0u;
        __syncthreads();
        uint32_t e = 0u;
        const int64_t n_words = (n_live + tp.bm_samples - 1) / tp.bm_samples;
        const uint32_t* ew = esc_bm + (int64_t)tp.bm_idx[l] * tp.bm_blocks;
        for (int64_t w = threadIdx.x; w < n_words; w += kBwdThreads) e |= ew[w];
        if (e) esc_bm_any = 1u;
        __syncthreads();
        by_bitmap = esc_bm_any == 0u;
    }
    // (the wave's number through readfirstlane: the queue's address stays on the scalar unit, see enqueue1)
    uint32_t* queue = reinterpret_cast<uint32_t*>(lds_tile + 2 * kTileEntries) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kQueueCap;
    if (by_bitmap && hashed) bwd_stream_bitmap<FIXED, false>(cx, lds_tile, queue, bitmaps + (int64_t)(tp.bm_row[l] + (int)t) * tp.bm_row_words, x01, g_l, n_live);
    else if (by_bitmap) bwd_stream_bitmap<FIXED, true>(cx, lds_tile, queue, bitmaps + (int64_t)(tp.bm_row[l] + (int)t) * tp.bm_row_words, x01, g_l, n_live);
    else if (coded && hashed && n_tiles <= (uint32_t)kMaskTiles) bwd_stream_bits<FIXED>(cx, lds_tile, queue, codes + (int64_t)tp.code_slot[l] * tp.n_pad + (int64_t)t * bit_row_words(n), x01, g_l, n_live, rep, R);
    else if (coded && hashed) bwd_stream_codes<FIXED, false>(cx, lds_tile, queue, codes + (int64_t)tp.code_slot[l] * tp.n_pad, x01, g_l, n_live, rep, R);
    else if (coded) bwd_stream_codes<FIXED, true>(cx, lds_tile, queue, codes + (int64_t)tp.code_slot[l] * tp.n_pad, x01, g_l, n_live, rep, R);
    else if (hashed) bwd_stream<FIXED, true>(cx, lds_tile, x01, g_l, n_live, rep, R);
    else bwd_stream<FIXED, false>(cx, lds_tile, x01, g_l, n_live, rep, R, tp.run_merge != 0);
    __syncthreads();
    int32_t field_max = 0;
    // ---- write back: local slot j of tile t is entry e(j)
    const float2* src = reinterpret_cast<const float2*>(lds_tile);
    float2* out = (R > 1) ? ws + tp.ws_off[l] + (int64_t)rep * size : grad + gp.offset[l];
    const bool acc = (R == 1) && tp.accumulate;
#ifdef PERF_BWD_BLOCK_TIMES         // (two workgroups per level report: a printf from every workgroup stretches the launch it measures)
    __syncthreads();
    if (FIXED && threadIdx.x == 0 && (t == 0u || t == n_tiles / 2u))
        printf("BLOCKT level %d tile %u rep %d of %d ticks %lld\n", l, t, rep, R, wall_clock64() - block_t0);
#endif
    // fixed point: replica slabs -- and, in raw mode, the table itself -- receive the integer fields, so that replicas
    // (and the ranks of a data-parallel step) are added up exactly, in any order
    const bool int_out = FIXED && (R > 1 || tp.raw_out);
    for (uint32_t j = threadIdx.x; j < (uint32_t)kTileEntries; j += kBwdThreads) {
        uint32_t e;
        if (hashed) e = t * (uint32_t)kTileEntries + j;
        else e = ((j / kChunk) * n_tiles + t) * kChunk + (j % kChunk);      // n_tiles is a power of two
        if (e >= size) continue;
        float2 v;
        if (FIXED) {
            const long long tot = (long long)lds64[j];
            const int32_t lo = (int32_t)(tot & 0xffffffffll);
            const int32_t hi = (int32_t)((tot - (long long)lo) >> 32);
            const int32_t alo = lo < 0 ? -(lo + 1) : lo, ahi = hi < 0 ? -(hi + 1) : hi;
            field_max = max(field_max, max(alo, ahi));
            if (int_out) { reinterpret_cast<int2*>(out)[e] = make_int2(lo, hi); continue; }
            v = make_float2((float)lo * from_fixed, (float)hi * from_fixed);
        } else {
            v = src[j];
        }
        if (acc) { const float2 o = out[e]; v.x += o.x; v.y += o.y; }
        out[e] = v;
    }
    // (a field that wrapped past +-2^31 reads back with an arbitrary value; the flag is global, so such a sum escapes only
    //  if NO field of ANY tile ends in the band [2^29, 2^32 - 2^29) -- i.e. if the largest sum of the whole table exceeds
    //  7x the level at which smaller sums already raise the flag while none of them lands there)
    if (FIXED && overflow_flag && field_max >= (1 << 29)) atomicOr(overflow_flag, 1);
    if (FIXED && hr_state && R == 1) {  // largest |field| of the level, for the feedback (ONE atomic per workgroup; replicated
                                        // levels report the max of their SUMMED fields from the reduction kernel)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) field_max = max(field_max, __shfl_xor(field_max, off));
        // The 24 maxima share a cache line, and read-modify-writes on one line retire one at a time, ~11 ns each.  A wave only
        // needs one when it RAISES the maximum -- but the look does not help when everybody finishes together: with a few
        // thousand live samples (the reference-faithful step) all 192 hashed owners end within a microsecond, their 3,072 waves
        // all read the stale zero and all queue: the launch took 41 us at 1,024 live samples against 12 us at none (rocprofv3,
        // tools/exp/bwd_live_sweep.py).  The workgroup's waves therefore agree on ONE value first (LDS) -- at most 192 atomics.
        __shared__ int32_t wave_max[kBwdThreads / 64];
        if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = field_max;
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t m = 0;
#pragma unroll
            for (int w = 0; w < kBwdThreads / 64; ++w) m = max(m, wave_max[w]);
            if (m > 0 && m > __hip_atomic_load(&hr_state[PERF_MAX_LEVELS + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&hr_state[PERF_MAX_LEVELS + l], m);
        }
    }
}

// Levels too large for LDS owners: plain scatter with global fp32 atomics (flat ~2e10/s on gfx950: a fallback for
// log2_hashmap_size >= 22, where 256+ owners per level would each have to walk every sample).  The level's slice of
// the gradient table is zeroed by the caller first unless it accumulates.
__global__ __launch_bounds__(256) void hashgrid_bwd_atomic_kernel(GridParams gp, uint32_t levels, const float* __restrict__ x01,
                                                                  const float2* __restrict__ dfeat, float* __restrict__ grad,
                                                                  int64_t n, const int64_t* __restrict__ n_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int l = blockIdx.y;
    if (i >= live_count(n, n_dev) || !((levels >> l) & 1u)) return;
    const float2 g = dfeat[(int64_t)l * n + i];
    if (g.x == 0.f && g.y == 0.f) return;
    const Corners c = corners_of(x01[3 * i], x01[3 * i + 1], x01[3 * i + 2], gp.scale[l], gp.res[l], gp.size[l], gp.hashed[l] != 0);
    float w[8];
    corner_weights(c.f, gp.interpolation == PERF_INTERP_SMOOTHSTEP, w);
    float* t = grad + 2 * gp.offset[l];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        unsafeAtomicAdd(t + 2 * (uint64_t)c.idx[k], w[k] * g.x);
        unsafeAtomicAdd(t + 2 * (uint64_t)c.idx[k] + 1, w[k] * g.y);
    }
}

// Fixed-point flavour of the fallback (the caller provides level_absmax and does not accumulate): the level's slice of the
// gradient table is used as an array of 64-bit words holding the same two signed 32-bit fixed-point fields as the LDS
// tiles -- ONE global atomic per corner instead of two, and integer sums: the result does not depend on the order the
// atomics retire in.  hashgrid_bwd_unfix_kernel turns the words into float2 in place.
__global__ __launch_bounds__(256) void hashgrid_bwd_atomic_fixed_kernel(GridParams gp, uint32_t levels, const float* __restrict__ x01,
                                                                        const float2* __restrict__ dfeat, float* __restrict__ grad,
                                                                        const float* __restrict__ level_absmax,
                                                                        const int32_t* __restrict__ hr_state, int64_t n,
                                                                        const int64_t* __restrict__ n_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int l = blockIdx.y;
    const int64_t n_live = live_count(n, n_dev);
    if (i >= n_live || !((levels >> l) & 1u)) return;
    const float2 g = dfeat[(int64_t)l * n + i];
    if (g.x == 0.f && g.y == 0.f) return;
    const float to_fixed = ldexpf(1.0f, fixed_point_shift(level_absmax[l], n_live, gp.size[l], hr_state, l));
    const Corners c = corners_of(x01[3 * i], x01[3 * i + 1], x01[3 * i + 2], gp.scale[l], gp.res[l], gp.size[l], gp.hashed[l] != 0);
    float w[8];
    corner_weights(c.f, gp.interpolation == PERF_INTERP_SMOOTHSTEP, w);
    if (gp.hashed[l] && c.cell[0] < (uint32_t)(kTileEntries - 1)) {
        // the association of the tile owners (apply_pairs: x-weight times the (y,z) product), so that a level adds up the same
        // integers whether its owners read bitmaps or -- workspace too small for them -- this scatter runs
        float fx = c.f[0], fy = c.f[1], fz = c.f[2];
        if (gp.interpolation == PERF_INTERP_SMOOTHSTEP) { fx = fx * fx * (3.0f - 2.0f * fx); fy = fy * fy * (3.0f - 2.0f * fy); fz = fz * fz * (3.0f - 2.0f * fz); }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float wyz = (((k >> 1) & 1) ? fy : 1.0f - fy) * ((k >> 2) ? fz : 1.0f - fz);
            w[k] = ((k & 1) ? fx : 1.0f - fx) * wyz;
        }
    }
    unsigned long long* t = reinterpret_cast<unsigned long long*>(grad) + gp.offset[l];
    const float sx = g.x * to_fixed, sy = g.y * to_fixed;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long v = ((long long)__float2int_rn(w[k] * sy) << 32) + (long long)__float2int_rn(w[k] * sx);
        atomicAdd(t + c.idx[k], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void hashgrid_bwd_unfix_kernel(GridParams gp, uint32_t levels, float* __restrict__ grad,
                                                                 const float* __restrict__ level_absmax, int32_t* __restrict__ hr_state,
                                                                 int32_t* __restrict__ overflow_flag, int64_t n,
                                                                 const int64_t* __restrict__ n_dev) {
    const int l = blockIdx.y;
    if (!((levels >> l) & 1u)) return;
    const uint32_t size = gp.size[l];
    const float from_fixed = ldexpf(1.0f, -fixed_point_shift(level_absmax[l], live_count(n, n_dev), size, hr_state, l));
    unsigned long long* t = reinterpret_cast<unsigned long long*>(grad) + gp.offset[l];
    int32_t field_max = 0;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < size; e += gridDim.x * 256) {
        const long long tot = (long long)t[e];
        if (tot == 0) continue;                          // (0 is 0.0f, 0.0f: untouched entries need no store)
        const int32_t lo = (int32_t)(tot & 0xffffffffll);
        const int32_t hi = (int32_t)((tot - (long long)lo) >> 32);
        reinterpret_cast<float2*>(t)[e] = make_float2((float)lo * from_fixed, (float)hi * from_fixed);
        const int32_t alo = lo < 0 ? -(lo + 1) : lo, ahi = hi < 0 ? -(hi + 1) : hi;
        field_max = max(field_max, max(alo, ahi));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) field_max = max(field_max, __shfl_xor(field_max, off));
    if ((threadIdx.x & 63) == 0 && field_max > 0) {
        if (overflow_flag && field_max >= (1 << 29)) atomicOr(overflow_flag, 1);
        if (hr_state) atomicMax(&hr_state[PERF_MAX_LEVELS + l], field_max);
    }
}

__host__ __device__ inline int reduce_blocks_of(uint32_t size, int width) {
    const uint32_t want = (size + 1023u) / 1024u;
    return (int)(want < (uint32_t)width ? (want > 0u ? want : 1u) : (uint32_t)width);
}

// sum the replica slabs (ws[level][replica][entry]) of the replicated (coarse) levels into the gradient table; the
// workgroup that finishes last applies the headroom feedback (hr_state: [adjustments][largest fields][done counter])
__global__ __launch_bounds__(256) void hashgrid_bwd_reduce_kernel(GridParams gp, TileParams tp, const float2* __restrict__ ws,
                                                                  float2* __restrict__ grad, int32_t* __restrict__ hr_state,
                                                                  const int32_t* __restrict__ shifts, int fixed,
                                                                  int32_t* __restrict__ overflow_flag, int n_ticket_blocks,
                                                                  RiderCountJob count, unsigned rider_cols) {
    // stage B of the step riders (step_riders_device.hpp) in the first `rider_cols` columns of every row: the next batch's counting pass
    if (blockIdx.x < rider_cols) {
        const unsigned b = blockIdx.y * rider_cols + blockIdx.x;
        if (b < (unsigned)count.n_blocks) rider_count_block(count, (int)b);
        return;
    }
    const unsigned bx = blockIdx.x - rider_cols;
    const int width = (int)(gridDim.x - rider_cols);
    const int l = blockIdx.y;
    const int R = tp.replicas_of[l];
    // (rows of levels without replicas have nothing to add up: they leave at once, without a ticket -- same-address atomics
    //  retire at ~11 ns each; with no replicated level at all, workgroup (0, 0) applies the feedback)
    if (R <= 1 && !(n_ticket_blocks == 0 && bx == 0 && blockIdx.y == 0)) return;
    // a replicated level takes one workgroup per 1,024 entries (at most the grid's width): the smallest ones must not pay -- in
    // tickets -- for the width the largest one needs (reduce_blocks_of() is what the host counted)
    if (R > 1 && (int)bx >= reduce_blocks_of(gp.size[l], width)) return;
    int sink = 0;
    if (R > 1) {
        const uint32_t size = gp.size[l];
        const float from_fixed = fixed ? ldexpf(1.0f, -shifts[l]) : 1.0f;
        int32_t field_max = 0;
        const uint32_t stride = (uint32_t)reduce_blocks_of(size, width) * 256;
        if (fixed) {
            // Four entries x four slabs per round trip: a thread of the largest replicated level owns a dozen entries, and
            // written as "for entry: for slab: load, add" every one of its 4 R loads was a round trip of its own (14 us for a
            // few megabytes).  Indices are clamped so that all sixteen loads are unconditional; integer sums, any order.
            const int2* p = reinterpret_cast<const int2*>(ws + tp.ws_off[l]);
            for (uint32_t e0 = bx * 256 + threadIdx.x; e0 < size; e0 += 4 * stride) {
                int32_t sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
                uint32_t ej[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) ej[j] = min(e0 + (uint32_t)j * stride, size - 1u);
                for (int r = 0; r < R; r += 4) {
                    int2 v[4][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int64_t slab = (int64_t)min(r + q, R - 1) * size;
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[q][j] = p[slab + ej[j]];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (r + q < R) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) { sx[j] += v[q][j].x; sy[j] += v[q][j].y; }
                        }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t e = e0 + (uint32_t)j * stride;
                    if (e >= size) break;
                    float2* o = grad + gp.offset[l] + e;
                    const int32_t ax = sx[j] < 0 ? -(sx[j] + 1) : sx[j], ay = sy[j] < 0 ? -(sy[j] + 1) : sy[j];
                    field_max = max(field_max, max(ax, ay));
                    if (tp.raw_out) { *reinterpret_cast<int2*>(o) = make_int2(sx[j], sy[j]); continue; }
                    float fx = (float)sx[j] * from_fixed, fy = (float)sy[j] * from_fixed;
                    if (tp.accumulate) { const float2 c = *o; fx += c.x; fy += c.y; }
                    *o = make_float2(fx, fy);
                }
            }
        } else {
            for (uint32_t e = bx * 256 + threadIdx.x; e < size; e += stride) {
                float2* o = grad + gp.offset[l] + e;
                const float2* p = ws + tp.ws_off[l] + e;
                float sx = 0.f, sy = 0.f;
                int r = 0;
                for (; r + 4 <= R; r += 4) {        // (loads in flight together, additions in slab order as before)
                    const float2 v0 = p[(int64_t)r * size], v1 = p[(int64_t)(r + 1) * size], v2 = p[(int64_t)(r + 2) * size],
                                 v3 = p[(int64_t)(r + 3) * size];
                    sx += v0.x; sy += v0.y; sx += v1.x; sy += v1.y; sx += v2.x; sy += v2.y; sx += v3.x; sy += v3.y;
                }
                for (; r < R; ++r) { const float2 v = p[(int64_t)r * size]; sx += v.x; sy += v.y; }
                if (tp.accumulate) { const float2 c = *o; sx += c.x; sy += c.y; }
                *o = make_float2(sx, sy);
            }
        }
        if (fixed) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) field_max = max(field_max, __shfl_xor(field_max, off));
            if ((threadIdx.x & 63) == 0 && field_max > 0) {
                if (overflow_flag && field_max >= (1 << 29)) atomicOr(overflow_flag, 1);
                // a RETURNING device-scope atomic: the wave waits until it has been performed at the memory side, so the
                // ticket below is ordered behind it without an agent-scope fence (which writes back the XCD's L2: ~20 us
                // over the 128 workgroups of this kernel, measured).  Only a wave that RAISES the level's maximum needs it
                // (same-address read-modify-writes retire one at a time, ~11 ns each; a look costs an L2 read).
                if (hr_state && field_max > __hip_atomic_load(&hr_state[PERF_MAX_LEVELS + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    sink = __hip_atomic_fetch_max(&hr_state[PERF_MAX_LEVELS + l], field_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (!hr_state) return;
    // ---- headroom feedback by the last workgroup of the replicated rows to get here
    __shared__ int last_block;
    if (n_ticket_blocks > 0) {
        asm volatile("" : : "v"(sink));                    // (uses the atomic's return value: the wave waits for it)
        __syncthreads();
        if (threadIdx.x == 0) last_block = (atomicAdd(&hr_state[2 * PERF_MAX_LEVELS], 1) == n_ticket_blocks - 1) ? 1 : 0;
        __syncthreads();
        if (!last_block) return;
    }
    if ((int)threadIdx.x < gp.n_levels) {
        const int fm = atomicMax(&hr_state[PERF_MAX_LEVELS + threadIdx.x], 0);     // (an atomic read: the value sits at the memory side)
        hr_state[threadIdx.x] = headroom_feedback(hr_state[threadIdx.x], fm);
        hr_state[PERF_MAX_LEVELS + threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) hr_state[2 * PERF_MAX_LEVELS] = 0;
}

}  // namespace perf

using namespace perf;

namespace perf {
__global__ void step_book_keep_flag_kernel(perf_step_book b) { step_bookkeeping_thread(b, false); }
}  // namespace perf
static void launch_step_book_keep_flag(const perf_step_book& b, void* stream) {
    hipLaunchKernelGGL(perf::step_book_keep_flag_kernel, dim3(1), dim3(1), 0, as_stream(stream), b);
}

// levels whose owners can run the coded variant (multi-tile levels); returns their number
static int plan_codes(const GridParams& gp, int64_t n, TileParams* tp) {
    int slots = 0;
    for (int l = 0; l < PERF_MAX_LEVELS; ++l) {
        tp->code_slot[l] = -1;
        if (l >= gp.n_levels || n >= kMaxCodedSamples || ((tp->bitmap_levels >> l) & 1u)) continue;
        const int64_t nt = tp->tiles_of[l];         // (plan_tiles ran before)
        // (at most 2^24 entries either way: the owners' 24-bit index arithmetic, see kMaxCodedHashedTiles)
        if (gp.hashed[l] ? (nt >= 2 && nt <= kMaxCodedHashedTiles && gp.res[l] + 2u < (uint32_t)kTileEntries) : (nt >= 2 && nt <= kMaxCodedDenseTiles)) {
            tp->code_slot[l] = slots++;
        }
    }
    tp->n_pad = (n + 3) & ~(int64_t)3;
    return slots;
}

// the coded levels as the pre-pass reads them (CodeLevel), in level order
static void plan_code_levels(const GridParams& gp, const TileParams& tp, CodePlan* cp) {
    *cp = CodePlan{};
    for (int l = 0; l < gp.n_levels; ++l) {
        if (tp.code_slot[l] < 0) continue;
        CodeLevel& d = cp->lv[cp->n_coded++];
        const uint32_t kind = gp.hashed[l] ? (tp.tiles_of[l] <= kMaskTiles ? kCodeMasks : kCodeBytes)
                                           : (gp.res[l] <= kPackedMaxRes ? kCodeDense : kCodeDenseWide);
        d.scale = gp.scale[l];
        d.kind_level = kind | ((uint32_t)l << 8);
        d.last = gp.size[l] - 1u;
        d.res = gp.res[l]; d.res2 = gp.res[l] * gp.res[l];
        d.tmask = (uint32_t)tp.tiles_of[l] - 1u;         // (plan_codes: 2..64 tiles)
        d.row = (int64_t)tp.code_slot[l] * tp.n_pad;
        for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t off = (c & 1u) * d.res + (c >> 1) * d.res2;
            d.off5 |= (off % kChunk) << (8 * c);
            d.offc |= ((off / kChunk) & 63u) << (8 * c);
            d.tmask4 |= d.tmask << (8 * c);
        }
    }
}

constexpr int64_t kShiftBytes = 256;        // per-level shifts the owners leave for the replica reduction

// bitmap rows of the levels plan_tiles marked (bitmap_levels); returns the bytes of [bitmaps][escape words] or 0
constexpr int64_t kBitmapMaxBytes = (int64_t)2 << 30;
static int64_t plan_bitmaps(const GridParams& gp, int64_t n, TileParams* tp, int* n_levels_out) {
    int rows = 0, idx = 0;
    for (int l = 0; l < PERF_MAX_LEVELS; ++l) {
        tp->bm_row[l] = -1; tp->bm_idx[l] = -1;
        if (l < gp.n_levels && ((tp->bitmap_levels >> l) & 1u)) { tp->bm_row[l] = rows; tp->bm_idx[l] = idx++; rows += tp->tiles_of[l]; }
    }
    int nt_max = 1;
    for (int l = 0; l < gp.n_levels; ++l) if ((tp->bitmap_levels >> l) & 1u) nt_max = tp->tiles_of[l] > nt_max ? tp->tiles_of[l] : nt_max;
    int samples = 1024;
    while (samples > 256 && (int64_t)nt_max * samples / 8 > 65536) samples >>= 1;
    tp->bm_samples = samples;
    tp->bm_blocks = div_up(n, samples);
    tp->bm_row_words = tp->bm_blocks * (samples / 32);
    *n_levels_out = idx;
    return (int64_t)rows * tp->bm_row_words * 4 + (int64_t)idx * tp->bm_blocks * 4;
}

// The ONE layout of a call's workspace: [replica slabs][shifts][tile codes][escape words][bitmaps][their escape words].  The size
// query returns `total`; the call takes the offsets and decides from workspace_bytes / alignment which optional sections it uses (a
// workspace WITHOUT room for the codes / bitmaps selects the position-streaming owners / the global-atomics scatter: how the tests
// reach those paths).  n == 0 asks for the minimum: slabs and shifts.  bm_bytes == 0: no plan with bitmap levels on offer.
struct BwdLayout { int64_t shifts_at, codes_at, esc_words, bits_at, bm_bytes, total; };

static BwdLayout plan_layout(const GridParams& gp, int64_t n) {
    BwdLayout L{};
    TileParams tp; int nb, bm_levels = 0; int64_t w, slab_entries = 0;
    const int bm_tiles = n < kMaxCodedSamples ? kBitmapMaxTiles : 0;
    for (int plan = 0; plan < 4; ++plan) {      // slabs: the largest of the plans a call may pick (both modes, without / with bitmap levels)
        plan_tiles(gp, (plan & 1) != 0, &tp, &nb, &w, (plan & 2) ? bm_tiles : 0);
        if (w > slab_entries) slab_entries = w;
    }
    L.shifts_at = (slab_entries * (int64_t)sizeof(float2) + 15) & ~(int64_t)15;
    L.codes_at = L.shifts_at + kShiftBytes;
    L.esc_words = div_up(n, kCodeSamplesPerBlock);
    // tp: the fixed-point plan with bitmap levels (tiles, code slots and bitmap rows are those of the fp32 plan: only the replicas differ)
    int slots = plan_codes(gp, n, &tp);
    if (n > 0 && tp.bitmap_levels) L.bm_bytes = plan_bitmaps(gp, n, &tp, &bm_levels);
    if (L.bm_bytes > kBitmapMaxBytes) L.bm_bytes = 0;
    if (tp.bitmap_levels && !L.bm_bytes) {      // no bitmaps: the call plans without them, and more levels take tile codes
        plan_tiles(gp, true, &tp, &nb, &w, 0);
        slots = plan_codes(gp, n, &tp);
    }
    const int64_t code_bytes = (int64_t)slots * tp.n_pad * 4 + (slots ? L.esc_words * 4 : 0);
    L.bits_at = (L.codes_at + code_bytes + 15) & ~(int64_t)15;
    L.total = slab_entries * (int64_t)sizeof(float2) + 16 + kShiftBytes + code_bytes + (L.bm_bytes ? L.bm_bytes + 16 : 0);
    return L;
}

extern "C" int64_t perf_hashgrid_bwd_workspace_bytes(const perf_grid_desc* grid, int64_t n) {
    GridParams gp;
    if (fill_params(grid, &gp)) return -1;
    return plan_layout(gp, n).total;
}

extern "C" int perf_hashgrid_bwd(const perf_grid_desc* grid, const float* x01, const float* dfeat,
                                 float* grad_table, int64_t n, const int64_t* n_dev, int accumulate, const float* level_absmax,
                                 int32_t* overflow_flag, int32_t* headroom_state, const int32_t* shifts_dev, int raw_fields,
                                 const int32_t* redo_flag, void* workspace, int64_t workspace_bytes, void* stream) {
    return perf_internal_hashgrid_bwd(grid, x01, dfeat, grad_table, n, n_dev, accumulate, level_absmax, overflow_flag, headroom_state, shifts_dev,
                                      raw_fields, redo_flag, workspace, workspace_bytes, stream, nullptr, nullptr);
}

// job (perf_field_bwd): the deferred second stage of the MLP backward that produced `dfeat` / `level_absmax`; it rides in the
// tile-code launch when there is one and gets a launch of its own otherwise -- in either case BEFORE the owners, which read level_absmax
int perf_internal_hashgrid_bwd(const perf_grid_desc* grid, const float* x01, const float* dfeat,
                               float* grad_table, int64_t n, const int64_t* n_dev, int accumulate, const float* level_absmax,
                               int32_t* overflow_flag, int32_t* headroom_state, const int32_t* shifts_dev, int raw_fields,
                               const int32_t* redo_flag, void* workspace, int64_t workspace_bytes, void* stream, const MlpReduceJob* job_in,
                               const perf_step_book* book) {
    return perf_internal_hashgrid_bwd_riders(grid, x01, dfeat, grad_table, n, n_dev, accumulate, level_absmax, overflow_flag, headroom_state, shifts_dev,
                                             raw_fields, redo_flag, workspace, workspace_bytes, stream, job_in, book, nullptr, nullptr);
}

namespace perf {
// a rider whose host launch does not take place: a launch of its own at the same place of the stream
__global__ __launch_bounds__(PERF_RIDER_THREADS) void rider_draw_kernel(RiderDrawJob j) { rider_draw_block(j, (int)blockIdx.x); }
__global__ __launch_bounds__(PERF_RIDER_THREADS) void rider_count_kernel(RiderCountJob j) { rider_count_block(j, (int)blockIdx.x); }
}  // namespace perf

// draw / count (perf_field_bwd_riders): stages A and B of the step riders -- A in the tile-code launch, B in the replica reduction
int perf_internal_hashgrid_bwd_riders(const perf_grid_desc* grid, const float* x01, const float* dfeat,
                                      float* grad_table, int64_t n, const int64_t* n_dev, int accumulate, const float* level_absmax,
                                      int32_t* overflow_flag, int32_t* headroom_state, const int32_t* shifts_dev, int raw_fields,
                                      const int32_t* redo_flag, void* workspace, int64_t workspace_bytes, void* stream, const MlpReduceJob* job_in,
                                      const perf_step_book* book, const RiderDrawJob* draw_in, const RiderCountJob* count_in) {
    RiderDrawJob draw{};
    RiderCountJob count{};
    if (draw_in) draw = *draw_in;
    if (count_in) count = *count_in;
    PERF_REQUIRE(!(redo_flag && (draw.n_blocks || count.n_blocks)), "perf_hashgrid_bwd: a redo call carries no riders");
    PERF_REQUIRE(!book || redo_flag, "perf_hashgrid_bwd: the bookkeeping rides in a repair launch only");
    MlpReduceJob job{};
    if (job_in) job = *job_in;
    GridParams gp;
    int rc = fill_params(grid, &gp);
    if (rc) return rc;
    PERF_REQUIRE(!(redo_flag && job.n_blocks), "perf_hashgrid_bwd: a redo call carries no deferred work");
    PERF_REQUIRE(grad_table, "NULL pointer");
    PERF_REQUIRE(n == 0 || (x01 && dfeat), "NULL pointer");
    const bool fixed = level_absmax != nullptr || shifts_dev != nullptr;
    if (redo_flag) {
        // The repair of a fixed-point call whose fields overflowed: ONE launch, predicated on the device flag, fp32 LDS
        // accumulation, every tile owned by a single workgroup that streams positions (no pre-pass, no replica reduction: the
        // slow-but-simple owners; the launch is a no-op dispatch in all but a handful of steps per million).
        PERF_REQUIRE(!fixed && !accumulate && !raw_fields, "perf_hashgrid_bwd: a redo call is an fp32, overwriting call");
        TileParams rp;
        int nb = 0;
        int64_t wse = 0;
        plan_tiles(gp, false, &rp, &nb, &wse, 0, true);
        if (rp.atomic_levels != 0u || nb == 0) { set_error("perf_hashgrid_bwd: the redo launch serves grids whose levels all fit LDS owners (<= 255 hashed / 64 dense tiles)"); return PERF_E_UNSUPPORTED; }
        rp.accumulate = 0; rp.raw_out = 0; rp.run_merge = 0; rp.n_pad = 0;
        for (int l = 0; l < PERF_MAX_LEVELS; ++l) rp.code_slot[l] = -1;
        const int lds_b = 2 * kTileEntries * (int)sizeof(float) + (kBwdThreads / 64) * kQueueCap * (int)sizeof(uint32_t);
        static std::once_flag redo_once;
        std::call_once(redo_once, [&]() {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&hashgrid_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_b);
        });
        if (n > 0)
            hashgrid_bwd_kernel<false><<<dim3(nb), dim3(kBwdThreads), lds_b, as_stream(stream)>>>(
                gp, rp, x01, (const float2*)dfeat, (float2*)grad_table, nullptr, nullptr, nullptr, headroom_state, nullptr, nullptr,
                nullptr, nullptr, nullptr, nullptr, n, n_dev, redo_flag, book ? *book : perf_step_book{}, book ? 1 : 0);
        else if (book)      // (no repair launch to ride in: the bookkeeping's own launch, the flag left for the caller all the same)
            launch_step_book_keep_flag(*book, stream);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(redo)");
        return PERF_OK;
    }
    PERF_REQUIRE(!shifts_dev || !headroom_state, "perf_hashgrid_bwd: given units (shifts_dev) exclude the headroom feedback");
    PERF_REQUIRE(!raw_fields || (fixed && !accumulate), "perf_hashgrid_bwd: raw fields need the fixed-point mode and accumulate == 0");
    TileParams tp;
    int n_blocks = 0;
    int64_t ws_entries = 0;
    const bool aligned_ws = (reinterpret_cast<uintptr_t>(workspace) & 15) == 0;
    const BwdLayout lay = plan_layout(gp, n);
    const int64_t shifts_at = lay.shifts_at, codes_at = lay.codes_at, esc_words = lay.esc_words, bits_at = lay.bits_at;
    // levels of 256..2048 tiles take LDS owners fed by per-tile bitmaps when the workspace holds the bitmaps, global atomics otherwise
    const bool use_bitmaps = aligned_ws && lay.bm_bytes && workspace_bytes >= bits_at + lay.bm_bytes;
    int bm_levels = 0;
    plan_tiles(gp, fixed, &tp, &n_blocks, &ws_entries, use_bitmaps ? kBitmapMaxTiles : 0);
    PERF_REQUIRE(!(raw_fields || shifts_dev) || tp.atomic_levels == 0u,
                 "perf_hashgrid_bwd: raw fields / given units are not available for levels on the global-atomics scatter (more than 2048 tiles, or no room for the per-tile bitmaps in the workspace)");
    tp.run_merge = 1;
    tp.accumulate = accumulate;
    tp.raw_out = raw_fields ? 1 : 0;
    PERF_REQUIRE(workspace && workspace_bytes >= shifts_at + kShiftBytes,
                 "perf_hashgrid_bwd: workspace too small (need %lld bytes)", (long long)(shifts_at + kShiftBytes));
    int32_t* shifts_ws = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + shifts_at);
    // tile codes of the multi-tile levels (workspace permitting)
    const int slots = plan_codes(gp, n, &tp);
    // (a slot holds a block's sixteen 32-byte pieces whole only from 256 rows on, see bit_row_words: below that the bit-row levels'
    //  slots stay unused)
    for (int l = 0; l < gp.n_levels; ++l)
        if (n < kCodeSamplesPerBlock && gp.hashed[l] && tp.tiles_of[l] <= kMaskTiles) tp.code_slot[l] = -1;
    uint32_t* codes = nullptr;
    uint32_t* escape = nullptr;
    uint32_t* bitmaps = nullptr;
    uint32_t* esc_bm = nullptr;
    if (tp.bitmap_levels) {
        (void)plan_bitmaps(gp, n, &tp, &bm_levels);
        bitmaps = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + bits_at);
        int rows = 0, nt_max = 0;
        for (int l = 0; l < gp.n_levels; ++l)
            if ((tp.bitmap_levels >> l) & 1u) { rows += tp.tiles_of[l]; nt_max = tp.tiles_of[l] > nt_max ? tp.tiles_of[l] : nt_max; }
        esc_bm = bitmaps + (int64_t)rows * tp.bm_row_words;
        static std::once_flag bm_once;
        std::call_once(bm_once, [&]() {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_bitmap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        });
        tile_bitmap_kernel<<<dim3((unsigned)tp.bm_blocks, (unsigned)bm_levels), dim3(256), (size_t)nt_max * (tp.bm_samples / 8), as_stream(stream)>>>(
            gp, tp, x01, (const float2*)dfeat, bitmaps, esc_bm, n, n_dev);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(bitmaps)");
    }
    if (slots > 0 && n > 0 && aligned_ws &&
        workspace_bytes >= codes_at + (int64_t)slots * tp.n_pad * 4 + esc_words * 4) {
        codes = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + codes_at);
        escape = codes + (int64_t)slots * tp.n_pad;
        CodePlan cp;
        plan_code_levels(gp, tp, &cp);
        const unsigned own = (unsigned)esc_words, all = (unsigned)draw.n_blocks + own + (unsigned)job.n_blocks;       // (codes: 16-byte aligned, as the workspace and codes_at are)
        tile_codes4_kernel<<<dim3(all), dim3(64 * kCodeWaves), 0, as_stream(stream)>>>(cp, x01, (const float2*)dfeat, codes, escape, n, n_dev, job, own, draw);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(codes)");
        job.n_blocks = 0;                          // (done)
        draw.n_blocks = 0;
    } else {
        for (int l = 0; l < PERF_MAX_LEVELS; ++l) tp.code_slot[l] = -1;
    }
    if (job.n_blocks) {                            // no tile-code launch to ride in
        perf_internal_launch_mlp_reduce(job, stream);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(deferred MLP reduce)");
    }
    if (draw.n_blocks) {
        rider_draw_kernel<<<dim3((unsigned)draw.n_blocks), dim3(PERF_RIDER_THREADS), 0, as_stream(stream)>>>(draw);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(stage A of its own)");
    }
    const int lds_bytes = 2 * kTileEntries * (int)sizeof(float) + (kBwdThreads / 64) * kQueueCap * (int)sizeof(uint32_t);
    static std::once_flag attr_once;                // one-time kernel attribute setup, safe under concurrent callers
    std::call_once(attr_once, [&]() {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&hashgrid_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&hashgrid_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    });
    if (n_blocks == 0) {
        // every level goes through the atomics fallback
    } else if (fixed)
        hashgrid_bwd_kernel<true><<<dim3(n_blocks), dim3(kBwdThreads), lds_bytes, as_stream(stream)>>>(
            gp, tp, x01, (const float2*)dfeat, (float2*)grad_table, (float2*)workspace, level_absmax, overflow_flag, headroom_state,
            shifts_dev, shifts_ws, codes, escape, bitmaps, esc_bm, n, n_dev, nullptr, perf_step_book{}, 0);
    else
        hashgrid_bwd_kernel<false><<<dim3(n_blocks), dim3(kBwdThreads), lds_bytes, as_stream(stream)>>>(
            gp, tp, x01, (const float2*)dfeat, (float2*)grad_table, (float2*)workspace, nullptr, nullptr, nullptr, nullptr, nullptr,
            codes, escape, bitmaps, esc_bm, n, n_dev, nullptr, perf_step_book{}, 0);
    PERF_LAUNCH_CHECK("perf_hashgrid_bwd");
    if (tp.atomic_levels && n > 0) {
        if (!accumulate)
            for (int l = 0; l < gp.n_levels; ++l)
                if ((tp.atomic_levels >> l) & 1u)
                    PERF_REQUIRE(hipMemsetAsync(grad_table + 2 * gp.offset[l], 0, (size_t)gp.size[l] * 2 * sizeof(float), as_stream(stream)) == hipSuccess,
                                 "perf_hashgrid_bwd: memset failed");
        if (level_absmax && !accumulate && (reinterpret_cast<uintptr_t>(grad_table) & 7) == 0) {      // fixed point: one 64-bit atomic per corner, order independent
            hashgrid_bwd_atomic_fixed_kernel<<<dim3((unsigned)div_up(n, 256), gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                gp, tp.atomic_levels, x01, (const float2*)dfeat, grad_table, level_absmax, headroom_state, n, n_dev);
            PERF_LAUNCH_CHECK("perf_hashgrid_bwd(atomics, fixed point)");
            hashgrid_bwd_unfix_kernel<<<dim3(1024, gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                gp, tp.atomic_levels, grad_table, level_absmax, headroom_state, overflow_flag, n, n_dev);
            PERF_LAUNCH_CHECK("perf_hashgrid_bwd(unfix)");
        } else {
            hashgrid_bwd_atomic_kernel<<<dim3((unsigned)div_up(n, 256), gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                gp, tp.atomic_levels, x01, (const float2*)dfeat, grad_table, n, n_dev);
            PERF_LAUNCH_CHECK("perf_hashgrid_bwd(atomics)");
        }
    } else if (tp.atomic_levels && !accumulate) {
        for (int l = 0; l < gp.n_levels; ++l)
            if ((tp.atomic_levels >> l) & 1u) (void)hipMemsetAsync(grad_table + 2 * gp.offset[l], 0, (size_t)gp.size[l] * 2 * sizeof(float), as_stream(stream));
    }
    const bool adapt = level_absmax && headroom_state && (n_blocks > 0 || (tp.atomic_levels && n > 0 && !accumulate));
    if (ws_entries > 0 || adapt) {      // replica sums, and the headroom feedback by the last workgroup
        constexpr int kReduceBlocks = 64;
        int n_tickets = 0;
        for (int l = 0; l < gp.n_levels; ++l) n_tickets += tp.replicas_of[l] > 1 ? reduce_blocks_of(gp.size[l], kReduceBlocks) : 0;
        // (stage B's workgroups: the first columns of every row, see the kernel)
        const unsigned rider_cols = (unsigned)div_up(count.n_blocks, gp.n_levels);
        hashgrid_bwd_reduce_kernel<<<dim3(rider_cols + kReduceBlocks, gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
            gp, tp, (const float2*)workspace, (float2*)grad_table, adapt ? headroom_state : nullptr,
            shifts_dev ? shifts_dev : shifts_ws, fixed ? 1 : 0, overflow_flag, n_tickets, count, rider_cols);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(reduce)");
        count.n_blocks = 0;
    }
    if (count.n_blocks) {
        rider_count_kernel<<<dim3((unsigned)count.n_blocks), dim3(PERF_RIDER_THREADS), 0, as_stream(stream)>>>(count);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd(stage B of its own)");
    }
    return PERF_OK;
}
