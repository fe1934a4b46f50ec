// Instantiation unit of mlp_device.hpp: the forward kernels that read their features through a row index (mlp_fwd_kernel<..., ROWS>),
// and their entry point perf_mlp_fwd_rows (include/perf_hip_pair.h).
#include "mlp_device.hpp"
#include "../../include/perf_hip_pair.h"

using namespace perf;

extern "C" int perf_mlp_fwd_rows(const perf_mlp_desc* mlp, const void* w16, const void* feat16, const int32_t* feat_index, int64_t feat_stride,
                                 const uint8_t* sel, float* out, int64_t n, const int64_t* n_dev, int dtype, void* stream) {
    int nh, ks;
    int rc = check_mlp(mlp, &nh, &ks);
    if (rc) return rc;
    PERF_REQUIRE(n >= 0, "perf_mlp_fwd_rows: n < 0");
    if (n == 0) return PERF_OK;
    PERF_REQUIRE(w16 && feat16 && feat_index && out, "perf_mlp_fwd_rows: NULL pointer");
    PERF_REQUIRE(feat_stride >= 1, "perf_mlp_fwd_rows: feat_stride < 1");
    PERF_REQUIRE(dtype == PERF_DTYPE_BF16 || dtype == PERF_DTYPE_FP16, "perf_mlp_fwd_rows: bad dtype %d", dtype);
    MlpParams mp{mlp->n_levels, mlp->n_out, mlp->out_act, mlp->exp_shift};
    const int blocks = mlp_blocks(n, nh == 1 ? 4 : 3);          // (perf_mlp_fwd's)
    if (dtype == PERF_DTYPE_BF16)
        dispatch_fwd_rows<BF16>(nh, ks, blocks, as_stream(stream), mp, (const uint16_t*)w16, (const uint32_t*)feat16, feat_index, feat_stride, sel, out, n, n_dev);
    else
        dispatch_fwd_rows<FP16>(nh, ks, blocks, as_stream(stream), mp, (const uint16_t*)w16, (const uint32_t*)feat16, feat_index, feat_stride, sel, out, n, n_dev);
    PERF_LAUNCH_CHECK("perf_mlp_fwd_rows");
    return PERF_OK;
}
