// The host checks every mesh unit's entry points begin with: the caller's workspace and the counts of the mesh.  No kernel lives here, so
// a unit that scans nothing (meshcolor.hip, meshray.hip) includes this header alone; the others get it through mesh_scan_device.hpp.
#pragma once
#include "common.hpp"

namespace perf {

// need: what the unit's perf_*_workspace_bytes returns for the call's sizes
static int workspace_check(const char* who, int64_t need, const void* workspace, int64_t workspace_bytes) {
    PERF_REQUIRE(workspace, "%s: NULL workspace", who);
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    PERF_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", who, (long long)workspace_bytes, (long long)need);
    return PERF_OK;
}

// the counts of a mesh against a unit's limits; faces_limit says the face limit in the unit's words ("2^38", "2^31 - 1", ...)
static int mesh_counts_check(const char* who, int64_t n_vertices, int64_t n_faces, int64_t max_vertices, int64_t max_faces, const char* faces_limit) {
    PERF_REQUIRE(n_vertices >= 0, "%s: a negative number of vertices (%lld)", who, (long long)n_vertices);
    PERF_REQUIRE(n_faces >= 0, "%s: a negative number of faces (%lld)", who, (long long)n_faces);
    PERF_REQUIRE(n_vertices <= max_vertices, "%s: %lld vertices are more than 2^30 (vertex indices are int32)", who, (long long)n_vertices);
    PERF_REQUIRE(n_faces <= max_faces, "%s: %lld faces are more than %s", who, (long long)n_faces, faces_limit);
    return PERF_OK;
}

}  // namespace perf
