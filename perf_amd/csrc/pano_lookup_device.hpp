// The look-up of a point in a registered panorama, stated once for the reprojection test (visibility.hip), the cull (meshvis.hip) and the
// colouring (meshcolor.hip): fp32, one rounding per operation in this order, so the three agree bit for bit.  It comes in two parts -- the
// pixel, then the bilinear tap of the distance map -- because the colouring keeps the taps and weights the other two throw away.
#pragma once
#include "common.hpp"

namespace perf {

// where a point falls in a panorama: its distance in the panorama's frame, the four corners of its bilinear cell and their weights
struct PanoPixel {
    float dist;
    int x0, y0, x1, y1;
    float wx0, wx1, wy0, wy1;
};

// rt = R^T (row major), t = the camera centre, h x w = the panorama's distance map
__device__ __forceinline__ PanoPixel pano_pixel(float x, float y, float z, const float (&rt)[9], const float (&t)[3], int32_t h, int32_t w) {
    const float px = sub_rn(x, t[0]), py = sub_rn(y, t[1]), pz = sub_rn(z, t[2]);
    // apply_rot(p - t, R^T): matmul row by row (utils/camera_utils.py:44-46)
    float l[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) l[a] = add_rn(add_rn(mul_rn(rt[3 * a], px), mul_rn(rt[3 * a + 1], py)), mul_rn(rt[3 * a + 2], pz));
    const float dist = sqrtf(add_rn(add_rn(mul_rn(l[0], l[0]), mul_rn(l[1], l[1])), mul_rn(l[2], l[2])));
    float d[3] = {__fdiv_rn(l[0], dist), __fdiv_rn(l[1], dist), __fdiv_rn(l[2], dist)};
    // direction_to_img_coord normalises once more
    const float nn = sqrtf(add_rn(add_rn(mul_rn(d[0], d[0]), mul_rn(d[1], d[1])), mul_rn(d[2], d[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = __fdiv_rn(d[a], nn);
    const float kPi = 3.14159265358979323846f;
    const float beta = asinf(d[2]), alpha = atan2f(d[1], d[0]);
    const float row = add_rn(__fdiv_rn(-beta, kPi), 0.5f);
    const float col = add_rn(-__fdiv_rn(alpha, mul_rn(2.0f, kPi)), 0.5f);
    // img_coord_to_sample_coord: x = col*2-1, y = row*2-1; grid_sample (align_corners=False): ix = ((x+1)*W - 1)/2, border = clamp
    const float gx = sub_rn(mul_rn(col, 2.0f), 1.0f), gy = sub_rn(mul_rn(row, 2.0f), 1.0f);
    float ix = __fdiv_rn(sub_rn(mul_rn(add_rn(gx, 1.0f), (float)w), 1.0f), 2.0f);
    float iy = __fdiv_rn(sub_rn(mul_rn(add_rn(gy, 1.0f), (float)h), 1.0f), 2.0f);
    ix = fminf(fmaxf(ix, 0.0f), (float)(w - 1));            // (a NaN becomes 0: fmaxf returns the other operand)
    iy = fminf(fmaxf(iy, 0.0f), (float)(h - 1));
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    PanoPixel p;
    p.dist = dist;
    p.x0 = (int)fx0; p.y0 = (int)fy0;
    p.x1 = p.x0 + 1; p.y1 = p.y0 + 1;
    p.wx1 = sub_rn(ix, fx0); p.wy1 = sub_rn(iy, fy0); p.wx0 = sub_rn(1.0f, p.wx1); p.wy0 = sub_rn(1.0f, p.wy1);
    return p;
}

// the bilinear tap of the distance map at the pixel, in torch's accumulation order: nw, ne, sw, se
__device__ __forceinline__ float pano_tap(const float* __restrict__ dmap, int32_t h, int32_t w, const PanoPixel& p) {
    auto at = [&](int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? dmap[(int64_t)yy * w + xx] : 0.0f; };
    float proj = mul_rn(at(p.y0, p.x0), mul_rn(p.wx0, p.wy0));
    proj = add_rn(proj, mul_rn(at(p.y0, p.x1), mul_rn(p.wx1, p.wy0)));
    proj = add_rn(proj, mul_rn(at(p.y1, p.x0), mul_rn(p.wx0, p.wy1)));
    proj = add_rn(proj, mul_rn(at(p.y1, p.x1), mul_rn(p.wx1, p.wy1)));
    return proj;
}

}  // namespace perf
