// TriMesh plumbing kernels (gfx950): face areas, packed <-> padded copies, index conversion and upload.
// (The regularisers live in mesh_losses.hip, the element-wise updates in mesh_update.hip.)
//
// Face areas are a gather over packed arrays: HBM/L2-bandwidth bound.  The reference does the gathers with
// `verts[:, faces]` temporaries (src/rep/mesh.jl:772).  Arithmetic order follows the reference expression by expression,
// unfused (-ffp-contract=off).
#include <cmath>

#include "fx3d_common.h"
#include "mesh_host.h"
#include "mesh_reg.h"

using namespace fx3d;

namespace {

constexpr int kThreads = kMeshThreads;

// (round 4) Both gather kernels below ran one element per thread and iteration: index load -> vertex gathers -> arithmetic, two
// dependent round trips per element and 15-22 elements per thread at a 4 M-face mesh (3.2 / 2.1 TB/s of algorithmic bytes,
// profiles/r04_*_hbm_roofline.txt).  Four elements per iteration now: every index first, then every gather, then the
// arithmetic (the expressions are unchanged: same bits per element).
struct __attribute__((packed, aligned(4))) I3 { int32_t a, b, c; };  // one face of a (3, F) index array: a 12-byte load
__device__ __forceinline__ float tri_area_p(const P3 &v1, const P3 &v2, const P3 &v3) {
    const float t1[3] = {v1.x, v1.y, v1.z}, t2[3] = {v2.x, v2.y, v2.z}, t3[3] = {v3.x, v3.y, v3.z};
    return tri_area(t1, t2, t3);
}
using meshreg::xcd_logical_block;  // (mesh_reg.h)

__global__ __launch_bounds__(kThreads) void faces_areas_packed_kernel(
    const float *__restrict__ verts, const int32_t *__restrict__ faces, long long F,
    float *__restrict__ areas) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long f0 = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + threadIdx.x; f0 < F; f0 += 4 * stride) {
        I3 fc[4];
        P3 v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long f = f0 + u * stride;
            fc[u] = *reinterpret_cast<const I3 *>(faces + 3 * (f < F ? f : f0));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u][0] = *reinterpret_cast<const P3 *>(verts + 3ll * fc[u].a);
            v[u][1] = *reinterpret_cast<const P3 *>(verts + 3ll * fc[u].b);
            v[u][2] = *reinterpret_cast<const P3 *>(verts + 3ll * fc[u].c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long f = f0 + u * stride;
            if (f < F) areas[f] = tri_area_p(v[u][0], v[u][1], v[u][2]);
        }
    }
}

__global__ __launch_bounds__(kThreads) void faces_areas_padded_kernel(
    const float *__restrict__ verts_padded, int Vmax, const int32_t *__restrict__ faces_padded,
    int Fmax, const int32_t *__restrict__ faces_len, int B, float *__restrict__ areas) {
    const long long total = (long long)B * Fmax;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < total;
         k += (long long)gridDim.x * kThreads) {
        const int b = (int)(k / Fmax), f = (int)(k % Fmax);
        float a = 0.0f;  // _packed_to_padded pad value 0 (src/rep/mesh.jl:806)
        if (f < faces_len[b]) {
            const int32_t *fc = faces_padded + 3 * k;
            const float *vb = verts_padded + (size_t)b * Vmax * 3;
            a = tri_area(vb + 3ll * fc[0], vb + 3ll * fc[1], vb + 3ll * fc[2]);
        }
        areas[k] = a;
    }
}

}  // namespace

extern "C" {

fx3d_status fx3d_faces_areas_packed(const float *verts, int64_t V, const int32_t *faces, int64_t F,
                                    float *areas, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && faces && areas, "fx3d_faces_areas_packed: null pointer");
    FX3D_REQUIRE(V > 0 && F > 0 && V < (1ll << 31), "fx3d_faces_areas_packed: bad sizes V=%lld F=%lld",
                 (long long)V, (long long)F);
    ProfileScope prof("faces_areas", as_stream(s));
    hipLaunchKernelGGL(faces_areas_packed_kernel, dim3(mesh_grid_for(F)), dim3(kThreads), 0, as_stream(s),
                       verts, faces, (long long)F, areas);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_faces_areas_padded(const float *verts_padded, int32_t Vmax,
                                    const int32_t *faces_padded, int32_t Fmax,
                                    const int32_t *faces_len, int32_t B, float *areas,
                                    fx3d_stream_t s) {
    FX3D_REQUIRE(verts_padded && faces_padded && faces_len && areas, "fx3d_faces_areas_padded: null pointer");
    FX3D_REQUIRE(Vmax > 0 && Fmax > 0 && B > 0, "fx3d_faces_areas_padded: bad sizes");
    hipLaunchKernelGGL(faces_areas_padded_kernel, dim3(mesh_grid_for((long long)B * Fmax)), dim3(kThreads),
                       0, as_stream(s), verts_padded, Vmax, faces_padded, Fmax, faces_len, B, areas);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_packed_to_padded(const float *packed, const int64_t *verts_len_host, int32_t B, int32_t Vmax,
                                  float *padded, fx3d_stream_t s) {
    FX3D_REQUIRE(packed && verts_len_host && padded && B > 0 && Vmax > 0, "fx3d_packed_to_padded: bad argument");
    hipStream_t st = as_stream(s);
    FX3D_FILL(padded, 0, sizeof(float) * 3 * (size_t)Vmax * B, st);  // pad value 0
    size_t cur = 0;
    for (int b = 0; b < B; ++b) {
        const size_t n = (size_t)verts_len_host[b];
        FX3D_REQUIRE(n <= (size_t)Vmax, "fx3d_packed_to_padded: mesh %d longer than Vmax", b);
        if (n) FX3D_HIP(hipMemcpyAsync(padded + (size_t)b * Vmax * 3, packed + cur * 3, n * 12, hipMemcpyDeviceToDevice, st));
        cur += n;
    }
    return FX3D_OK;
}

fx3d_status fx3d_padded_to_packed(const float *padded, const int64_t *verts_len_host, int32_t B, int32_t Vmax,
                                  float *packed, fx3d_stream_t s) {
    FX3D_REQUIRE(packed && verts_len_host && padded && B > 0 && Vmax > 0, "fx3d_padded_to_packed: bad argument");
    hipStream_t st = as_stream(s);
    size_t cur = 0;
    for (int b = 0; b < B; ++b) {
        const size_t n = (size_t)verts_len_host[b];
        FX3D_REQUIRE(n <= (size_t)Vmax, "fx3d_padded_to_packed: mesh %d longer than Vmax", b);
        if (n) FX3D_HIP(hipMemcpyAsync(packed + cur * 3, padded + (size_t)b * Vmax * 3, n * 12, hipMemcpyDeviceToDevice, st));
        cur += n;
    }
    return FX3D_OK;
}

}  // extern "C"

// ---- the reference's index arrays -> int32 0-based on the device (include/flux3d_hip.h: fx3d_index_convert) -----------------
namespace {
template <typename IT>
__global__ __launch_bounds__(kThreads) void index_convert_kernel(const IT *__restrict__ src, long long n, long long base, int clamp_pad,
                                                                 long long limit, int32_t *__restrict__ dst, unsigned int *bad) {
    unsigned int nbad = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        long long v = (long long)src[i] - base;
        if (v < 0 && clamp_pad) v = 0;  // padding
        else if (limit > 0 ? (v < 0 || v >= limit) : (v < -2147483648ll || v > 2147483647ll)) { v = 0; ++nbad; }  // (no limit: still an int32)
        dst[i] = (int32_t)v;
    }
    if (bad && nbad) atomicAdd(bad, nbad);
}
size_t index_elem_bytes(int t) { return t == FX3D_IDX_I64 ? 8 : 4; }
}  // namespace

extern "C" {

fx3d_status fx3d_index_convert(const void *src_dev, int32_t index_type, int32_t index_base, int64_t count, int32_t clamp_pad,
                               int64_t limit, int32_t *dst_dev, uint32_t *bad_dev, fx3d_stream_t s) {
    FX3D_REQUIRE(index_type == FX3D_IDX_I32 || index_type == FX3D_IDX_U32 || index_type == FX3D_IDX_I64,
                 "fx3d_index_convert: index_type %d (FX3D_IDX_I32 / _U32 / _I64)", index_type);
    FX3D_REQUIRE(count >= 0 && limit >= 0 && limit <= (1ll << 31), "fx3d_index_convert: bad count / limit");
    if (count == 0) return FX3D_OK;
    FX3D_REQUIRE(src_dev && dst_dev, "fx3d_index_convert: null pointer");
    // a range check whose violations nobody can see would rewrite corrupt indices to vertex 0 in silence
    FX3D_REQUIRE(limit == 0 || bad_dev, "fx3d_index_convert: limit > 0 needs bad_dev (a zeroed device counter of the violations)");
    hipStream_t st = as_stream(s);
    const dim3 g(mesh_grid_for(count)), b(kThreads);
    if (index_type == FX3D_IDX_I64)
        hipLaunchKernelGGL(index_convert_kernel<long long>, g, b, 0, st, static_cast<const long long *>(src_dev), (long long)count,
                           (long long)index_base, clamp_pad, (long long)limit, dst_dev, bad_dev);
    else if (index_type == FX3D_IDX_U32)
        hipLaunchKernelGGL(index_convert_kernel<unsigned int>, g, b, 0, st, static_cast<const unsigned int *>(src_dev), (long long)count,
                           (long long)index_base, clamp_pad, (long long)limit, dst_dev, bad_dev);
    else
        hipLaunchKernelGGL(index_convert_kernel<int>, g, b, 0, st, static_cast<const int *>(src_dev), (long long)count,
                           (long long)index_base, clamp_pad, (long long)limit, dst_dev, bad_dev);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_index_upload_workspace_bytes(int32_t index_type, int64_t count, size_t *bytes) {
    FX3D_REQUIRE(bytes && count >= 0, "fx3d_index_upload_workspace_bytes: bad argument");
    FX3D_REQUIRE(index_type == FX3D_IDX_I32 || index_type == FX3D_IDX_U32 || index_type == FX3D_IDX_I64,
                 "fx3d_index_upload_workspace_bytes: index_type %d", index_type);
    *bytes = index_elem_bytes(index_type) * (size_t)count;
    return FX3D_OK;
}

fx3d_status fx3d_index_upload(const void *src_host, int32_t index_type, int32_t index_base, int64_t count, int32_t clamp_pad,
                              int64_t limit, int32_t *dst_dev, uint32_t *bad_dev, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    size_t need = 0;
    const fx3d_status rc = fx3d_index_upload_workspace_bytes(index_type, count, &need);
    if (rc) return rc;
    if (count == 0) return FX3D_OK;
    FX3D_REQUIRE(src_host && dst_dev, "fx3d_index_upload: null pointer");
    const fx3d_status wrc = ws_check("fx3d_index_upload", "workspace", ws, ws_bytes, need);
    if (wrc) return wrc;
    hipStream_t st = as_stream(s);
    FX3D_HIP(hipMemcpyAsync(ws, src_host, need, hipMemcpyHostToDevice, st));
    const fx3d_status crc = fx3d_index_convert(ws, index_type, index_base, count, clamp_pad, limit, dst_dev, bad_dev, s);
    if (crc) return crc;
    FX3D_HIP(hipStreamSynchronize(st));  // pageable host memory: blocking, like fx3d_memcpy_h2d
    return FX3D_OK;
}

}  // extern "C"
