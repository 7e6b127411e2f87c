// ScanNet mesh superpoints: the data-parallel steps of segmentator.segment_mesh(vertices, faces) [UPSTREAM ScanNet
// Segmentator], called at data/ScanNetV2/prepare_data_inst_ScanNetV2.py:77 and :157 -- face normals, vertex normals (a
// running mean over the incident face slots) and the weight of every face edge.  The definition is restated in DESIGN.md
// 4.17 (the external binary is not on hand); tests/mesh_segment_ref.py is its numpy form and these kernels equal it bit for
// bit: fp32 throughout, every product and sum its own rounding (the library is built -ffp-contract=off), the sums in the
// written order, `/` and sqrtf correctly rounded (hipcc's default).  The stable sort by weight is torch's; the two sweeps
// over the sorted edges are a serial recurrence and run on the host (wsis_host_mesh_merge, host_ops.cpp).
#include "common.h"

#include <cmath>

namespace wsis {
namespace {

constexpr int MS_BLOCK = 256;

struct F3 {
  float x, y, z;
};
__device__ __forceinline__ F3 ld3(const float* __restrict__ p, int64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ F3 sub3(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// a / |a|, 0 where the length is 0
__device__ __forceinline__ F3 unit3(F3 a) {
  const float len = sqrtf(dot3(a, a));
  if (len == 0.0f) return {0.0f, 0.0f, 0.0f};
  return {a.x / len, a.y / len, a.z / len};
}
__device__ __forceinline__ bool vertex_ok(int64_t i, int64_t V) { return i >= 0 && i < V; }

// thread i: vertex i is looked at for non-finite coordinates, face i gets its normal and its three CSR keys
__global__ __launch_bounds__(MS_BLOCK) void mesh_face_normals_kernel(const float* __restrict__ xyz, int64_t V,
                                                                     const int64_t* __restrict__ faces, int64_t F,
                                                                     float* __restrict__ fnormal, int64_t* __restrict__ keys,
                                                                     int32_t* __restrict__ err) {
  const int64_t n = F > V ? F : V;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < V) {
      const F3 p = ld3(xyz, i);
      if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) atomicAdd(err + 1, 1);
    }
    if (i < F) {
      int64_t v[3];
      int bad = 0;
      for (int s = 0; s < 3; ++s) {
        v[s] = faces[3 * i + s];
        if (!vertex_ok(v[s], V)) {
          v[s] = 0;
          ++bad;
        }
        keys[3 * i + s] = v[s];
      }
      if (bad) atomicAdd(err, bad);
      const F3 p1 = ld3(xyz, v[0]);
      const F3 a = sub3(ld3(xyz, v[1]), p1), b = sub3(ld3(xyz, v[2]), p1);
      const F3 c = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
      const F3 nf = unit3(c);
      fnormal[3 * i] = nf.x;
      fnormal[3 * i + 1] = nf.y;
      fnormal[3 * i + 2] = nf.z;
    }
  }
}

// one lane per vertex: the running mean is a recurrence over the row, in the row's (ascending face-slot) order
__global__ __launch_bounds__(MS_BLOCK) void mesh_vertex_normals_kernel(const float* __restrict__ fnormal,
                                                                       const int32_t* __restrict__ perm,
                                                                       const int32_t* __restrict__ off, int64_t V,
                                                                       float* __restrict__ vnormal) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    F3 n = {0.0f, 0.0f, 0.0f};
    float cnt = 0.0f;
    const int32_t end = off[v + 1];
    for (int32_t j = off[v]; j < end; ++j) {
      const F3 nf = ld3(fnormal, perm[j] / 3);
      const float r = 1.0f / (cnt + 1.0f);
      n.x = n.x + (nf.x - n.x) * r;
      n.y = n.y + (nf.y - n.y) * r;
      n.z = n.z + (nf.z - n.z) * r;
      cnt += 1.0f;
    }
    vnormal[3 * v] = n.x;
    vnormal[3 * v + 1] = n.y;
    vnormal[3 * v + 2] = n.z;
  }
}

// one thread per edge e = 3 f + slot
__global__ __launch_bounds__(MS_BLOCK) void mesh_edge_weights_kernel(const float* __restrict__ xyz,
                                                                     const float* __restrict__ vnormal, int64_t V,
                                                                     const int64_t* __restrict__ faces, int64_t E,
                                                                     int32_t* __restrict__ ea, int32_t* __restrict__ eb,
                                                                     float* __restrict__ ew) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = (uint32_t)e / 3u, slot = (uint32_t)e - 3u * f;      // E < 2^31
    int64_t v[3];
    for (int s = 0; s < 3; ++s) {
      v[s] = faces[3 * (int64_t)f + s];
      if (!vertex_ok(v[s], V)) v[s] = 0;
    }
    const int64_t a = slot == 2 ? v[2] : v[0], b = slot == 1 ? v[2] : v[1];
    const F3 d = unit3(sub3(ld3(xyz, b), ld3(xyz, a)));
    const F3 na = ld3(vnormal, a), nb = ld3(vnormal, b);
    const float dot = dot3(na, nb), dot2 = dot3(nb, d);
    float w = 1.0f - dot;
    if (dot2 > 0.0f) w = w * w;
    ea[e] = (int32_t)a;
    eb[e] = (int32_t)b;
    ew[e] = w;
  }
}

constexpr int64_t kInt32Limit = (int64_t)1 << 31;

}  // namespace
}  // namespace wsis

using namespace wsis;

extern "C" {

int wsis_mesh_face_normals(const float* d_vertices, int64_t V, const int64_t* d_faces, int64_t F, float* d_fnormal,
                           int64_t* d_keys, int32_t* d_err, void* stream) {
  WSIS_REQUIRE(V >= 0 && V < kInt32Limit && F >= 0 && 3 * F < kInt32Limit, "0 <= V < 2^31 and 0 <= 3 F < 2^31");
  WSIS_REQUIRE(d_err, "null error word");
  WSIS_REQUIRE(!(F > 0 && V == 0), "faces but no vertices");
  WSIS_REQUIRE((V == 0 || d_vertices) && (F == 0 || (d_faces && d_fnormal && d_keys)), "null pointer");
  hipStream_t st = as_stream(stream);
  WSIS_HIP_CHECK(hipMemsetAsync(d_err, 0, 2 * sizeof(int32_t), st));
  if (V == 0) return WSIS_OK;
  hipLaunchKernelGGL(mesh_face_normals_kernel, dim3(grid_for(F > V ? F : V, MS_BLOCK)), dim3(MS_BLOCK), 0, st, d_vertices, V,
                     d_faces, F, d_fnormal, d_keys, d_err);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_mesh_vertex_normals(const float* d_fnormal, const int32_t* d_perm, const int32_t* d_offsets, int64_t V, int64_t F,
                             float* d_vnormal, void* stream) {
  WSIS_REQUIRE(V >= 0 && V < kInt32Limit && F >= 0 && 3 * F < kInt32Limit, "0 <= V < 2^31 and 0 <= 3 F < 2^31");
  if (V == 0) return WSIS_OK;
  WSIS_REQUIRE(d_offsets && d_vnormal && (F == 0 || (d_fnormal && d_perm)), "null pointer");
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3(grid_for(V, MS_BLOCK)), dim3(MS_BLOCK), 0, as_stream(stream), d_fnormal,
                     d_perm, d_offsets, V, d_vnormal);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_mesh_edge_weights(const float* d_vertices, const float* d_vnormal, int64_t V, const int64_t* d_faces, int64_t F,
                           int32_t* d_a, int32_t* d_b, float* d_w, void* stream) {
  WSIS_REQUIRE(V >= 0 && V < kInt32Limit && F >= 0 && 3 * F < kInt32Limit, "0 <= V < 2^31 and 0 <= 3 F < 2^31");
  if (F == 0) return WSIS_OK;
  WSIS_REQUIRE(V > 0, "faces but no vertices");
  WSIS_REQUIRE(d_vertices && d_vnormal && d_faces && d_a && d_b && d_w, "null pointer");
  hipLaunchKernelGGL(mesh_edge_weights_kernel, dim3(grid_for(3 * F, MS_BLOCK)), dim3(MS_BLOCK), 0, as_stream(stream),
                     d_vertices, d_vnormal, V, d_faces, 3 * F, d_a, d_b, d_w);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
