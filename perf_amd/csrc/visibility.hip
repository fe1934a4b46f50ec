// Reprojection visibility tests around the renderer: NeRFScene.get_pano_visibility_mask
// (modules/scene/nerf.py:321-358) and SupInfoPool.geo_check (modules/dataset/sup_info.py:261-302).  Per pixel of a rendered
// panorama: back-projected point -> direction and distance in a registered panorama's frame -> equirect image coordinate
// (utils/camera_utils.py:134-151) -> bilinear look-up of that panorama's distance map with grid_sample's border padding /
// align_corners=False arithmetic (these steps are pano_lookup_device.hpp's, shared with the mesh cull and the mesh colouring)
// -> depth test, folded over the panoramas with max (visibility) or min (consistency).
// Then binary morphology with OpenCV's elliptical structuring elements.  One thread per pixel, fully coalesced; the
// reference runs ~15 torch kernels per registered panorama and two kornia convolutions.
#include "common.hpp"
#include "pano_lookup_device.hpp"

namespace perf {

struct PanoFrame { float rt[9]; float t[3]; };      // rt = R^T (row major), t = camera centre

__global__ __launch_bounds__(256) void pano_reproject_kernel(const float* __restrict__ pts, int64_t n, PanoFrame pf,
                                                             const float* __restrict__ dmap, int32_t h, int32_t w, int32_t mode,
                                                             float eps, float* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PanoPixel p = pano_pixel(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pf.rt, pf.t, h, w);
    const float dist = p.dist, proj = pano_tap(dmap, h, w, p);
    if (mode == 0) {            // visibility: seen by this panorama if not behind what it stored (+ 1/256)
        const float v = (dist < add_rn(proj, eps)) ? 1.0f : 0.0f;
        mask[i] = fmaxf(mask[i], v);
    } else {                    // consistency: the point must lie behind what this panorama stored
        const float v = (proj < dist) ? 1.0f : 0.0f;
        mask[i] = fminf(mask[i], v);
    }
}

struct Ellipse { uint32_t row_bits[16]; int32_t rows, cols; };

// op 0: dilation (outside the image = background), op 1: erosion (outside = foreground), both with the element's reflection
// handled by the caller's row masks; in/out are 0/1 floats
__global__ __launch_bounds__(256) void morph_kernel(const float* __restrict__ in, float* __restrict__ out, int32_t h, int32_t w,
                                                    Ellipse el, int32_t op) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)h * w) return;
    const int y = (int)(i / w), x = (int)(i % w);
    const int ry = el.rows / 2, rx = el.cols / 2;
    bool any = false, all = true;
    for (int dy = 0; dy < el.rows; ++dy)
        for (int dx = 0; dx < el.cols; ++dx) {
            if (!((el.row_bits[dy] >> dx) & 1u)) continue;
            const int yy = y + dy - ry, xx = x + dx - rx;
            const bool inside = yy >= 0 && yy < h && xx >= 0 && xx < w;
            const bool v = inside ? (in[(int64_t)yy * w + xx] > 0.5f) : (op == 1);
            any |= v; all &= v;
        }
    out[i] = (op == 0 ? any : all) ? 1.0f : 0.0f;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_pano_reproject(const float* pts, int64_t n, const float* pose, const float* distance_map, int32_t height,
                                   int32_t width, int32_t mode, float eps, float* mask, void* stream) {
    PERF_REQUIRE(n >= 0 && height >= 1 && width >= 1 && (mode == 0 || mode == 1), "perf_pano_reproject: bad arguments");
    if (n == 0) return PERF_OK;
    PERF_REQUIRE(pts && pose && distance_map && mask, "NULL pointer");
    PanoFrame pf;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) pf.rt[3 * a + b] = pose[4 * b + a];     // R^T
        pf.t[a] = pose[4 * a + 3];
    }
    hipLaunchKernelGGL(pano_reproject_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, as_stream(stream), pts, n, pf,
                       distance_map, height, width, mode, eps, mask);
    PERF_LAUNCH_CHECK("perf_pano_reproject");
    return PERF_OK;
}

extern "C" int perf_morph_binary(const float* in, float* out, int32_t height, int32_t width, const uint32_t* row_bits,
                                 int32_t rows, int32_t cols, int32_t op, void* stream) {
    PERF_REQUIRE(height >= 1 && width >= 1 && rows >= 1 && rows <= 16 && cols >= 1 && cols <= 32 && (op == 0 || op == 1),
                 "perf_morph_binary: bad arguments");
    PERF_REQUIRE(in && out && row_bits && in != out, "perf_morph_binary: NULL or aliased buffers");
    Ellipse el;
    for (int r = 0; r < 16; ++r) el.row_bits[r] = r < rows ? row_bits[r] : 0u;
    el.rows = rows; el.cols = cols;
    hipLaunchKernelGGL(morph_kernel, dim3((unsigned)div_up((int64_t)height * width, 256)), dim3(256), 0, as_stream(stream), in, out,
                       height, width, el, op);
    PERF_LAUNCH_CHECK("perf_morph_binary");
    return PERF_OK;
}
