// Vertex and face normals of a packed TriMesh (gfx950) and their adjoints w.r.t. the packed vertices:
// compute_verts_normals_packed / compute_faces_normals_packed (src/rep/mesh.jl:589-621, 689-699).
//
// What the reference computes on the CPU (include/flux3d_hip.h states the definition): every vertex takes, per corner row r,
// the cross product c_r of the HIGHEST-numbered face whose corner r it is (`A[:, I] = A[:, I] + X` with repeated I is last
// write wins), raw = ((+0 + c_0) + c_1) + c_2 with absent terms skipped, then _normalize.  The vertex -> (face, corner) table of
// fx3d_build_vertex_faces (entries face * 4 + corner, ascending per vertex) names the winners directly: the last entry with
// corner r.  A thread per vertex walks its entries, so no atomics and no memset anywhere: the forward's optional winner mask
// has every byte written by the one vertex that owns the (face, corner), and the adjoints are gathers in a fixed order.
// Arithmetic follows the reference expression by expression, unfused (-ffp-contract=off).
#include <cmath>

#include "fx3d_common.h"
#include "mesh_reg.h"

using namespace fx3d;

namespace {

constexpr int kThreads = 256;
constexpr int kFaceMaxBlocks = 4096;   // the face-parallel kernels grid-stride four faces at a time, as faces_areas_packed
constexpr float kEps = 1e-6f;          // _normalize's eps (src/rep/utils.jl:23-27), T.(1e-6) for T = Float32
constexpr int kChunk = 8;              // table entries a vertex thread requests at once (a sheet vertex has 6, a closed mesh ~6)

struct __attribute__((packed, aligned(4))) I3 { int32_t a, b, c; };  // one face of a (3, F) index array: a 12-byte load
using meshreg::xcd_logical_block;

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 sub3(const P3 &p, const P3 &q) { return F3{p.x - q.x, p.y - q.y, p.z - q.z}; }
// _lg_cross (src/rep/utils.jl:4-21): the operand order of tri_area (fx3d_common.h)
__device__ __forceinline__ F3 cross3(const F3 &a, const F3 &b) {
    return F3{(a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)};
}
// c_r(f) = _lg_cross(p[r+1] - p[r], p[r+2] - p[r]), corners cyclic (the three statements of src/rep/mesh.jl:603-614)
__device__ __forceinline__ F3 corner_cross(const P3 (&p)[3], int r) {
    const P3 &o = p[r], &u = p[r == 2 ? 0 : r + 1], &w = p[r == 0 ? 2 : r - 1];
    return cross3(sub3(u, o), sub3(w, o));
}
// _normalize(A; dims = 1) (src/rep/utils.jl:23-29): A ./ max(sqrt((x*x + y*y) + z*z), eps), with Julia's max (NaN wins; fmaxf
// would return eps).  *s: the norm.
__device__ __forceinline__ F3 normalize3(const F3 &c, float *s) {
    const float q = ((c.x * c.x) + (c.y * c.y)) + (c.z * c.z);
    const float sq = sqrtf(q);
    const float d = (sq > kEps || sq != sq) ? sq : kEps;
    *s = sq;
    return F3{c.x / d, c.y / d, c.z / d};
}
// g_raw = d normalize^T g at the normal n of norm s (include/flux3d_hip.h): s > eps: (g - n * ((n.x*g.x + n.y*g.y) + n.z*g.z)) / s,
// otherwise (eps is the max, or s is NaN) g / eps
__device__ __forceinline__ F3 normalize_bwd(const F3 &n, float s, const P3 &g) {
    if (s > kEps) {
        const float dot = ((n.x * g.x) + (n.y * g.y)) + (n.z * g.z);
        return F3{(g.x - (n.x * dot)) / s, (g.y - (n.y * dot)) / s, (g.z - (n.z * dot)) / s};
    }
    return F3{g.x / kEps, g.y / kEps, g.z / kEps};
}
// corner t's term of c_r's Jacobian transpose applied to g: for a = p[r+1] - p[r], b = p[r+2] - p[r], corner r+1 gets
// cross(b, g), corner r+2 gets cross(g, a), corner r their negated sum
__device__ __forceinline__ F3 corner_cross_bwd(const P3 (&p)[3], int r, int t, const F3 &g) {
    const P3 &o = p[r], &u = p[r == 2 ? 0 : r + 1], &w = p[r == 0 ? 2 : r - 1];
    const F3 a = sub3(u, o), b = sub3(w, o);
    const F3 da = cross3(b, g), db = cross3(g, a);
    if (t == r) return F3{-(da.x + db.x), -(da.y + db.y), -(da.z + db.z)};
    return t == (r == 2 ? 0 : r + 1) ? da : db;
}
__device__ __forceinline__ P3 load_p3(const float *__restrict__ a, long long i) { return *reinterpret_cast<const P3 *>(a + 3 * i); }

// The winning faces of vertex v per corner row (-1: v is never that corner) from its table entries; `mask` (optional): byte
// face * 3 + corner <- "this entry is the winner", for every entry of v.
__device__ __forceinline__ void vertex_winners(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ ent, long long v,
                                               int (&w)[3], unsigned char *__restrict__ mask) {
    w[0] = -1; w[1] = -1; w[2] = -1;
    const int e0 = rowptr[v], e1 = rowptr[v + 1];
    for (int c0 = e0; c0 < e1; c0 += kChunk) {
        int en[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) en[k] = ent[c0 + k < e1 ? c0 + k : e1 - 1];
#pragma unroll
        for (int k = 0; k < kChunk; ++k)  // ascending (face, corner): the last entry of a corner row wins
            if (c0 + k < e1) w[en[k] & 3] = en[k] >> 2;
    }
    if (mask)
        for (int e = e0; e < e1; ++e) {
            const int en = ent[e], f = en >> 2, t = en & 3;
            mask[3ll * f + t] = (unsigned char)(w[t] == f);
        }
}

// The raw (un-normalised) vertex normal from the winners: ((+0 + c_0(w_0)) + c_1(w_1)) + c_2(w_2), absent terms skipped.
__device__ __forceinline__ F3 vertex_raw(const float *__restrict__ verts, const int32_t *__restrict__ faces, const int (&w)[3]) {
    I3 fc[3];
    P3 p[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) fc[r] = *reinterpret_cast<const I3 *>(faces + 3ll * (w[r] >= 0 ? w[r] : 0));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p[r][0] = load_p3(verts, fc[r].a);
        p[r][1] = load_p3(verts, fc[r].b);
        p[r][2] = load_p3(verts, fc[r].c);
    }
    F3 raw{0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (w[r] >= 0) {
            const F3 c = corner_cross(p[r], r);
            raw.x = raw.x + c.x; raw.y = raw.y + c.y; raw.z = raw.z + c.z;
        }
    return raw;
}

// BWD = false: normals (3, V) and, if mask != nullptr, the winner mask.  BWD = true: g_raw (3, V) of the vertex normals for the
// incoming gradient gout (3, V).  A thread per vertex, grid-stride.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void verts_normals_kernel(const float *__restrict__ verts, long long V,
                                                                 const int32_t *__restrict__ faces, const int32_t *__restrict__ rowptr,
                                                                 const int32_t *__restrict__ ent, const float *__restrict__ gout,
                                                                 float *__restrict__ out, unsigned char *__restrict__ mask) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long v = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + threadIdx.x; v < V; v += stride) {
        int w[3];
        vertex_winners(rowptr, ent, v, w, BWD ? nullptr : mask);
        float s;
        const F3 n = normalize3(vertex_raw(verts, faces, w), &s);
        if (BWD) {
            const F3 g = normalize_bwd(n, s, load_p3(gout, v));
            *reinterpret_cast<P3 *>(out + 3 * v) = P3{g.x, g.y, g.z};
        } else {
            *reinterpret_cast<P3 *>(out + 3 * v) = P3{n.x, n.y, n.z};
        }
    }
}

// BWD = false: face normals (3, F).  BWD = true: g_raw (3, F) of the face normals for gout (3, F).  Four faces per thread and
// iteration: every index first, then every gather, then the arithmetic (faces_areas_packed_kernel, mesh.hip).
template <bool BWD>
__global__ __launch_bounds__(kThreads) void faces_normals_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                 long long F, const float *__restrict__ gout, float *__restrict__ out) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long f0 = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + threadIdx.x; f0 < F; f0 += 4 * stride) {
        I3 fc[4];
        P3 p[4][3], g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long f = f0 + u * stride;
            fc[u] = *reinterpret_cast<const I3 *>(faces + 3 * (f < F ? f : f0));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            p[u][0] = load_p3(verts, fc[u].a);
            p[u][1] = load_p3(verts, fc[u].b);
            p[u][2] = load_p3(verts, fc[u].c);
            if (BWD) {
                const long long f = f0 + u * stride;
                g[u] = load_p3(gout, f < F ? f : f0);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long f = f0 + u * stride;
            if (f >= F) continue;
            float s;
            const F3 n = normalize3(corner_cross(p[u], 0), &s);
            const F3 o = BWD ? normalize_bwd(n, s, g[u]) : n;
            *reinterpret_cast<P3 *>(out + 3 * f) = P3{o.x, o.y, o.z};
        }
    }
}

// The adjoints' gather: vertex u walks its entries (f, t) in ascending order and, for every role r of face f that counts --
// the mask's winners (vertex normals), role 0 of every face (face normals, mask == nullptr) -- adds corner t's term of c_r(f)'s
// Jacobian transpose applied to graw of the role's owner (the vertex faces[r, f] / the face f).  The sum starts from gverts[u]
// (accumulate) or +0 and is written once.  MASK: vertex normals (mask != nullptr), else face normals.
template <bool MASK>
__global__ __launch_bounds__(kThreads) void normals_bwd_gather_kernel(const float *__restrict__ verts, long long V,
                                                                      const int32_t *__restrict__ faces,
                                                                      const int32_t *__restrict__ rowptr, const int32_t *__restrict__ ent,
                                                                      const unsigned char *__restrict__ mask,
                                                                      const float *__restrict__ graw, float *__restrict__ gverts,
                                                                      int accumulate) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long u = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + threadIdx.x; u < V; u += stride) {
        F3 acc{0.0f, 0.0f, 0.0f};
        if (accumulate) {
            const P3 b = load_p3(gverts, u);
            acc = F3{b.x, b.y, b.z};
        }
        const int e0 = rowptr[u], e1 = rowptr[u + 1];
        for (int c0 = e0; c0 < e1; c0 += 4) {  // four entries in flight: entries, then faces and masks, then corners and graw
            int en[4];
            I3 fc[4];
            unsigned int mk[4];
            P3 p[4][3], g[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) en[k] = ent[c0 + k < e1 ? c0 + k : e1 - 1];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long f = en[k] >> 2;
                fc[k] = *reinterpret_cast<const I3 *>(faces + 3 * f);
                mk[k] = MASK ? (unsigned int)mask[3 * f] | ((unsigned int)mask[3 * f + 1] << 1) | ((unsigned int)mask[3 * f + 2] << 2) : 1u;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                p[k][0] = load_p3(verts, fc[k].a);
                p[k][1] = load_p3(verts, fc[k].b);
                p[k][2] = load_p3(verts, fc[k].c);
                if (MASK) {
                    const int32_t own[3] = {fc[k].a, fc[k].b, fc[k].c};
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        if (mk[k] & (1u << r)) g[k][r] = load_p3(graw, own[r]);
                } else {
                    g[k][0] = load_p3(graw, en[k] >> 2);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c0 + k >= e1) break;
                const int t = en[k] & 3;
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (mk[k] & (1u << r)) {
                        const F3 term = corner_cross_bwd(p[k], r, t, F3{g[k][r].x, g[k][r].y, g[k][r].z});
                        acc.x = acc.x + term.x; acc.y = acc.y + term.y; acc.z = acc.z + term.z;
                    }
            }
        }
        *reinterpret_cast<P3 *>(gverts + 3 * u) = P3{acc.x, acc.y, acc.z};
    }
}

// Grids: the vertex walks take a vertex per thread with no cap (the Laplacian adjoint's gather measured fastest that way,
// mesh_host.h: mesh_grid_for); the face kernels stop at 4096 blocks like faces_areas.  Option mesh_max_blocks != 0 caps both.
int grid_vertices(long long n) {
    long long g = (n + kThreads - 1) / kThreads;
    const int cap = opt(OPT_MESH_MAX_BLOCKS);
    if (cap > 0 && g > cap) g = cap;
    if (g > (1ll << 30)) g = 1ll << 30;
    return (int)(g < 1 ? 1 : g);
}
int grid_faces(long long n) {
    long long g = (n + kThreads - 1) / kThreads;
    int cap = opt(OPT_MESH_MAX_BLOCKS);
    if (cap < 1 || cap > kFaceMaxBlocks) cap = kFaceMaxBlocks;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

size_t ws_need(int64_t V, int64_t F) {
    const int64_t n = V > F ? V : F;
    WsBump ws;
    ws.put((size_t)n * 12);  // the raw gradients of the vertices or the faces
    return ws.at;
}

fx3d_status check_sizes(const char *fn, int64_t V, int64_t F) {
    FX3D_REQUIRE(V > 0 && F > 0 && V < (1ll << 31) && F < (1ll << 29), "%s: bad sizes V=%lld F=%lld", fn, (long long)V,
                 (long long)F);
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_normals_workspace_bytes(int64_t V, int64_t F, size_t *bytes) {
    FX3D_REQUIRE(bytes, "fx3d_normals_workspace_bytes: null output");
    const fx3d_status rc = check_sizes("fx3d_normals_workspace_bytes", V, F);
    if (rc) return rc;
    *bytes = ws_need(V, F);
    return FX3D_OK;
}

fx3d_status fx3d_verts_normals_packed(const float *verts, int64_t V, const int32_t *faces, int64_t F, const int32_t *vf_rowptr,
                                      const int32_t *vf_ent, float *normals, uint8_t *winner_mask, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && faces && vf_rowptr && vf_ent && normals, "fx3d_verts_normals_packed: null pointer");
    const fx3d_status rc = check_sizes("fx3d_verts_normals_packed", V, F);
    if (rc) return rc;
    ProfileScope prof("verts_normals", as_stream(s));
    hipLaunchKernelGGL(verts_normals_kernel<false>, dim3(grid_vertices(V)), dim3(kThreads), 0, as_stream(s), verts, (long long)V,
                       faces, vf_rowptr, vf_ent, nullptr, normals, winner_mask);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_verts_normals_bwd(const float *verts, int64_t V, const int32_t *faces, int64_t F, const int32_t *vf_rowptr,
                                   const int32_t *vf_ent, const uint8_t *winner_mask, const float *gout, float *gverts,
                                   int32_t accumulate, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && faces && vf_rowptr && vf_ent && winner_mask && gout && gverts, "fx3d_verts_normals_bwd: null pointer");
    const fx3d_status rc = check_sizes("fx3d_verts_normals_bwd", V, F);
    if (rc) return rc;
    if (!ws || ws_bytes < ws_need(V, F)) {
        set_error("fx3d_verts_normals_bwd: workspace too small (%zu < %zu)", ws_bytes, ws_need(V, F));
        return FX3D_ERR_WORKSPACE;
    }
    float *graw = static_cast<float *>(ws);
    hipStream_t st = as_stream(s);
    ProfileScope prof("verts_normals_bwd", st);
    hipLaunchKernelGGL(verts_normals_kernel<true>, dim3(grid_vertices(V)), dim3(kThreads), 0, st, verts, (long long)V, faces,
                       vf_rowptr, vf_ent, gout, graw, nullptr);
    FX3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(normals_bwd_gather_kernel<true>, dim3(grid_vertices(V)), dim3(kThreads), 0, st, verts, (long long)V, faces,
                       vf_rowptr, vf_ent, winner_mask, graw, gverts, (int)(accumulate != 0));
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_faces_normals_packed(const float *verts, int64_t V, const int32_t *faces, int64_t F, float *normals,
                                      fx3d_stream_t s) {
    FX3D_REQUIRE(verts && faces && normals, "fx3d_faces_normals_packed: null pointer");
    const fx3d_status rc = check_sizes("fx3d_faces_normals_packed", V, F);
    if (rc) return rc;
    ProfileScope prof("faces_normals", as_stream(s));
    hipLaunchKernelGGL(faces_normals_kernel<false>, dim3(grid_faces(F)), dim3(kThreads), 0, as_stream(s), verts, faces,
                       (long long)F, nullptr, normals);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_faces_normals_bwd(const float *verts, int64_t V, const int32_t *faces, int64_t F, const int32_t *vf_rowptr,
                                   const int32_t *vf_ent, const float *gout, float *gverts, int32_t accumulate, void *ws,
                                   size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && faces && vf_rowptr && vf_ent && gout && gverts, "fx3d_faces_normals_bwd: null pointer");
    const fx3d_status rc = check_sizes("fx3d_faces_normals_bwd", V, F);
    if (rc) return rc;
    if (!ws || ws_bytes < ws_need(V, F)) {
        set_error("fx3d_faces_normals_bwd: workspace too small (%zu < %zu)", ws_bytes, ws_need(V, F));
        return FX3D_ERR_WORKSPACE;
    }
    float *graw = static_cast<float *>(ws);
    hipStream_t st = as_stream(s);
    ProfileScope prof("faces_normals_bwd", st);
    hipLaunchKernelGGL(faces_normals_kernel<true>, dim3(grid_faces(F)), dim3(kThreads), 0, st, verts, faces, (long long)F, gout,
                       graw);
    FX3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(normals_bwd_gather_kernel<false>, dim3(grid_vertices(V)), dim3(kThreads), 0, st, verts, (long long)V, faces,
                       vf_rowptr, vf_ent, nullptr, graw, gverts, (int)(accumulate != 0));
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
