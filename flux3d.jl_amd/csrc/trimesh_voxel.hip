// trimesh_to_voxel / _voxelize (src/conversions.jl:133-207) for device-resident meshes.
//
// The reference voxelises every mesh i of the batch on its own (:133-145).  With v (3,V_i) the mesh's vertices -- all of
// them, also those no face uses -- and f (3,F_i) its faces:
//   1. verts = (v .- minimum(v)) ./ (maximum(v) - minimum(v)): ONE scalar min and max over all 3 V_i coordinates (:147-149),
//      Float32, a correctly rounded division.
//   2. points starts as all normalised vertices (:151).
//   3. Level by level over the triangle set (:158-197): side_k = sum((a .- b).^2, dims = 1) = ((dx*dx) + dy*dy) + dz*dz in
//      Float32, unfused (-ffp-contract=off in the Makefile); a triangle is kept iff max(side_1, side_2, side_3) >
//      (1.0/res)^2 -- a Float32 compared with a Float64 threshold, so the compare is done in double.  A kept triangle
//      adds its midpoints v4 = (v1+v3)/2, v5 = (v1+v2)/2, v6 = (v2+v3)/2 to points and is replaced by its children
//      (v1,v4,v5) (v5,v2,v6) (v5,v4,v6) (v4,v3,v6) (:171-196); a dropped triangle ends there.
//   4. idx = trunc(points * Float32(res-1)) (:198-203) and voxels[idx_x+1, idx_y+1, idx_z+1, i] = 1 (:204).  The x coordinate
//      indexes the FIRST (fastest) dimension: flat index ix + res*(iy + res*(iz + res*i)) -- the opposite of voxel.hip,
//      whose fastest dimension is the reference's innermost loop variable z.  The `(+res) % res` of :200-201 is a no-op:
//      normalised points lie in [0, 1].
// A triangle's fate depends on itself alone, so evaluating each face's subdivision tree by itself yields exactly the
// reference's point set; midpoints are commutative sums halved and (a-b)^2 == (b-a)^2, so the vertex roles do not change a bit.
// A mesh with zero extent or a NaN / Inf coordinate normalises to NaN, and the reference throws (round(Int, NaN) at :200).
// Here such a mesh (and one without vertices, or with a face id outside [0, V_i)) is COUNTED in *bad_dev (optional,
// caller-zeroed) and its grid is left zero; the wrappers raise when the count is non-zero.
//
// The work is badly unbalanced (a ModelNet mesh at res 32: thousands of faces that never split, a few that go 6 levels
// deep).  Midpoint children are the parent at half scale, so a node at level l has max side^2 ~ s0 / 4^l (s0: the root's):
//   launch 1  (one block per mesh)      the scalar range and the mesh's validity.
//   launch 2  (one block per 1024 faces)  each face's depth bound K_f (levels kept if the scaling were exact) and its
//             4^(K_f-1) leaf slots, one per node of the deepest kept level; their exclusive prefix within the block.
//   launch 3  (one block)                 the batch's items -- per mesh its vertices, then its face blocks' leaf slots --
//             as one int64 exclusive prefix; the grand total stays on the device, so nothing is read back and the call
//             can be captured into a graph.
//   launch 4  (grid-stride)               one item per vertex and per leaf slot, found by binary search in the two
//             prefixes.  A slot walks its base-4 path from the root with the reference's Float32 arithmetic, tests "kept"
//             at every level, and emits a node's three midpoints only when its remaining path digits are all zero (each
//             node exactly once).  The bound is an estimate: a path node that tests "dropped" ends the slot, and a slot
//             node that still tests "kept" explores its subtree depth first -- no work is ever dropped.
// Every write is a plain store of 1.0f into a grid zeroed by fill_bytes: no atomics, no float sums, deterministic.
#include "fx3d_common.h"
#include "scan_common.h"

namespace fx3d {
namespace {

constexpr int kPlanThreads = 1024;
constexpr int kSlotThreads = 256;
constexpr int kMaxSlotDigits = 12;  // 4^12 leaf slots per face at most; deeper trees continue depth first (never at res <= 1024)
constexpr int kMaxExtraDigits = 28;  // depth-first levels below a slot (normalised data: side^2 <= 3, thr >= 2^-20 -> <= 11 levels)

struct MeshInfo {
    float lo, span;
    int bad, pad;
};

struct V3 {
    float x, y, z;
};
struct Tri {
    V3 a, b, c;
};

__device__ __forceinline__ V3 load_norm(const float *__restrict__ p, float lo, float span) {
    return V3{(p[0] - lo) / span, (p[1] - lo) / span, (p[2] - lo) / span};  // (v .- verts_min) ./ (verts_max - verts_min)
}
__device__ __forceinline__ float side2(V3 a, V3 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;  // sum((a .- b) .^ 2, dims = 1), unfused
}
__device__ __forceinline__ bool kept(const Tri &t, double thr) {
    const float s = fmaxf(fmaxf(side2(t.a, t.b), side2(t.b, t.c)), side2(t.c, t.a));
    return (double)s > thr;  // sides .> smallest_side: Float32 promoted to Float64
}
__device__ __forceinline__ V3 mid(V3 a, V3 b) { return V3{(a.x + b.x) / 2.0f, (a.y + b.y) / 2.0f, (a.z + b.z) / 2.0f}; }
// child k of t: new_traingles = [1 4 5; 5 2 6; 5 4 6; 4 3 6] with v4 = (v1+v3)/2, v5 = (v1+v2)/2, v6 = (v2+v3)/2
__device__ __forceinline__ Tri child(const Tri &t, int k) {
    const V3 m4 = mid(t.a, t.c), m5 = mid(t.a, t.b), m6 = mid(t.b, t.c);
    switch (k) {
        case 0: return Tri{t.a, m4, m5};
        case 1: return Tri{m5, t.b, m6};
        case 2: return Tri{m5, m4, m6};
        default: return Tri{m4, t.c, m6};
    }
}
// K: the number of levels a face would keep if every child were its parent at exactly half scale.  thr and the scaling
// by 1/4 are exact in double, so launches 2 and 4 compute the same K from the same s0.
__device__ __forceinline__ int depth_bound(const Tri &t, double thr) {
    double s = (double)fmaxf(fmaxf(side2(t.a, t.b), side2(t.b, t.c)), side2(t.c, t.a));
    int K = 0;
    while (s > thr && K <= kMaxSlotDigits) {
        ++K;
        s *= 0.25;
    }
    return K;  // 0 .. kMaxSlotDigits + 1; slots = K ? 4^(K-1) : 0
}

// launch 1: block b = mesh b.  The scalar range and the mesh's validity.
__global__ __launch_bounds__(kPlanThreads) void tv_range_kernel(const float *__restrict__ verts, int Vmax,
                                                                const int32_t *__restrict__ verts_len,
                                                                MeshInfo *__restrict__ info, uint32_t *bad_dev) {
    const int b = blockIdx.x;
    const int Vb = min(max(verts_len[b], 0), Vmax);
    __shared__ float sw[2 * kPlanThreads / kWave];
    const Range r = block_range<kPlanThreads>(verts + (size_t)b * Vmax * 3, 3 * Vb, sw);
    if (threadIdx.x == 0) {
        // (a zero lo or hi may carry either sign: span is the same, and a vertex that normalises to -0.0 instead of +0.0
        //  gives the same sides (dx * dx), the same truncated index 0 and midpoints of the same value)
        const float span = r.hi - r.lo;
        // finite inputs with 0 < span < inf normalise into [0, 1]; anything else yields a NaN vertex (the reference throws)
        const bool bad = r.nan || Vb == 0 || !(span > 0.0f) || !(span <= 3.402823466e38f);
        info[b] = MeshInfo{r.lo, span, bad ? 1 : 0, 0};
        if (bad && bad_dev) atomicAdd(bad_dev, 1u);
    }
}

// launch 2: block (c, b) = faces [c*1024, (c+1)*1024) of mesh b.  Each face's leaf slots, their exclusive prefix within
// the chunk (face_off) and the chunk's total (chunk_tot).  A face id outside [0, V_b) makes the mesh bad (counted once).
__global__ __launch_bounds__(kPlanThreads) void tv_count_kernel(const float *__restrict__ verts, int Vmax,
                                                                const int32_t *__restrict__ verts_len,
                                                                const int32_t *__restrict__ faces, int Fmax,
                                                                const int32_t *__restrict__ faces_len, double thr,
                                                                MeshInfo *__restrict__ info, long long *__restrict__ face_off,
                                                                long long *__restrict__ chunk_tot, uint32_t *bad_dev) {
    __shared__ long long sw[kPlanThreads / kWave], stot;
    const int c = blockIdx.x, b = blockIdx.y, nch = gridDim.x;
    const MeshInfo mi = info[b];
    const int Vb = min(max(verts_len[b], 0), Vmax);
    const int Fb = min(max(faces_len[b], 0), Fmax);
    const int f = c * kPlanThreads + threadIdx.x;
    const float *vb = verts + (size_t)b * Vmax * 3;
    long long cnt = 0;
    int badface = 0;
    if (!mi.bad && f < Fb) {
        const int32_t *fi = faces + ((size_t)b * Fmax + f) * 3;
        const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
        if ((unsigned)i0 < (unsigned)Vb && (unsigned)i1 < (unsigned)Vb && (unsigned)i2 < (unsigned)Vb) {
            const Tri t{load_norm(vb + 3 * i0, mi.lo, mi.span), load_norm(vb + 3 * i1, mi.lo, mi.span),
                        load_norm(vb + 3 * i2, mi.lo, mi.span)};
            const int K = depth_bound(t, thr);
            cnt = K ? 1ll << (2 * (K - 1)) : 0;
        } else {
            badface = 1;
        }
    }
    const long long ex = block_exclusive_scan_serial(cnt, sw, &stot);
    if (f < Fb) face_off[(size_t)b * Fmax + f] = ex;
    if (__syncthreads_or(badface) && threadIdx.x == 0) {
        if (atomicExch(&info[b].bad, 1) == 0 && bad_dev) atomicAdd(bad_dev, 1u);  // the first to flag the mesh counts it
    }
    if (threadIdx.x == 0) chunk_tot[(size_t)b * nch + c] = stot;
}

// launch 3 (one block): the batch's items in order -- per mesh [its V_b vertices][chunk 0's leaf slots]...[chunk nch-1's]
// -- as one exclusive prefix over B * (nch + 1) entries (a bad mesh contributes nothing); start[B * (nch + 1)] = the total.
__global__ __launch_bounds__(kPlanThreads) void tv_scan_kernel(const int32_t *__restrict__ verts_len, int Vmax, int B,
                                                               int nch, const MeshInfo *__restrict__ info,
                                                               const long long *__restrict__ chunk_tot,
                                                               long long *__restrict__ start) {
    __shared__ long long sw[kPlanThreads / kWave], stot;
    const long long n = (long long)B * (nch + 1);
    long long carry = 0;
    for (long long base = 0; base < n; base += kPlanThreads) {
        const long long e = base + threadIdx.x;
        long long items = 0;
        if (e < n) {
            const int b = (int)(e / (nch + 1)), j = (int)(e % (nch + 1));
            if (!info[b].bad) items = j == 0 ? (long long)min(max(verts_len[b], 0), Vmax) : chunk_tot[(size_t)b * nch + j - 1];
        }
        const long long ex = block_exclusive_scan_serial(items, sw, &stot);
        if (e < n) start[e] = carry + ex;
        carry += stot;
    }
    if (threadIdx.x == 0) start[n] = carry;
}

__device__ __forceinline__ void put(float *__restrict__ vg, int res, float fr, V3 p, long long &last) {
    // trunc(points * Float32(res-1)) + 1 (:198-203); points lie in [0, 1], the clamp only guards the store
    const int ix = min(max((int)(p.x * fr), 0), res - 1);
    const int iy = min(max((int)(p.y * fr), 0), res - 1);
    const int iz = min(max((int)(p.z * fr), 0), res - 1);
    const long long o = ix + (long long)res * (iy + (long long)res * iz);
    if (o != last) vg[o] = 1.0f;  // consecutive points of one node often share a voxel
    last = o;
}
__device__ __forceinline__ void emit_mids(float *__restrict__ vg, int res, float fr, const Tri &t) {
    long long last = -1;
    put(vg, res, fr, mid(t.a, t.c), last);  // v4
    put(vg, res, fr, mid(t.a, t.b), last);  // v5
    put(vg, res, fr, mid(t.b, t.c), last);  // v6
}

// last index i in [0, n) with a[i] <= x (a non-decreasing, a[0] <= x)
__device__ __forceinline__ int last_le(const long long *__restrict__ a, int n, long long x) {
    int lo = 0, hi = n;  // invariant: a[lo] <= x, answer in [lo, hi)
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (a[m] <= x) lo = m;
        else hi = m;
    }
    return lo;
}

// launch 4: every vertex and leaf slot of the batch, grid-stride.
__global__ __launch_bounds__(kSlotThreads) void tv_slots_kernel(const float *__restrict__ verts, int Vmax,
                                                                const int32_t *__restrict__ verts_len,
                                                                const int32_t *__restrict__ faces, int Fmax,
                                                                const int32_t *__restrict__ faces_len, int B, int nch,
                                                                int res, double thr, const MeshInfo *__restrict__ info,
                                                                const long long *__restrict__ face_off,
                                                                const long long *__restrict__ start,
                                                                float *__restrict__ vox) {
    const int n = B * (nch + 1);
    const long long total = start[n];
    const long long stride = (long long)gridDim.x * kSlotThreads;
    const float fr = (float)(res - 1);
    const size_t cells = (size_t)res * res * res;
    for (long long g = (long long)blockIdx.x * kSlotThreads + threadIdx.x; g < total; g += stride) {
        const int e = last_le(start, n, g);  // empty entries share their start with the next one
        const int b = e / (nch + 1), j = e % (nch + 1);
        const MeshInfo mi = info[b];
        const float *vb = verts + (size_t)b * Vmax * 3;
        float *vg = vox + cells * b;
        const long long local = g - start[e];
        long long last = -1;
        if (j == 0) {  // points = verts (:151): every vertex, referenced or not
            put(vg, res, fr, load_norm(vb + 3 * local, mi.lo, mi.span), last);
            continue;
        }
        const int f0 = (j - 1) * kPlanThreads;  // a leaf slot of chunk j-1: its first face has offset 0 <= local
        const long long *fo = face_off + (size_t)b * Fmax + f0;
        const int f = f0 + last_le(fo, min(min(max(faces_len[b], 0), Fmax) - f0, kPlanThreads), local);
        const int32_t *fi = faces + ((size_t)b * Fmax + f) * 3;
        Tri t{load_norm(vb + 3 * fi[0], mi.lo, mi.span), load_norm(vb + 3 * fi[1], mi.lo, mi.span),
              load_norm(vb + 3 * fi[2], mi.lo, mi.span)};
        const int D = depth_bound(t, thr) - 1;  // path digits of this face's slots (>= 0: the face has slots)
        const long long slot = local - fo[f - f0];
        bool deeper = false;
        for (int l = 0;; ++l) {
            if (!kept(t, thr)) break;  // dropped: the subtree ends (its corners were emitted by its parent)
            const int rem = D - l;
            if ((slot & ((1ll << (2 * rem)) - 1)) == 0) emit_mids(vg, res, fr, t);  // each node once
            if (rem == 0) {
                deeper = true;
                break;
            }
            t = child(t, (int)((slot >> (2 * (rem - 1))) & 3));
        }
        if (!deeper) continue;
        // the slot's node is kept: its subtree goes on below the bound, depth first (digit e of the path at bits 2(e-1))
        unsigned long long path = 0;
        int d = 1;
        while (d > 0) {
            Tri u = t;
            for (int q = 1; q <= d; ++q) u = child(u, (int)((path >> (2 * (q - 1))) & 3));
            if (kept(u, thr)) {
                emit_mids(vg, res, fr, u);
                if (d < kMaxExtraDigits) {
                    ++d;  // descend to its first child (digit 0)
                    continue;
                }
            }
            while (d > 0 && ((path >> (2 * (d - 1))) & 3) == 3) {
                path &= ~(3ull << (2 * (d - 1)));
                --d;
            }
            if (d > 0) path += 1ull << (2 * (d - 1));
        }
    }
}

int chunks(int Fmax) { return (Fmax + kPlanThreads - 1) / kPlanThreads; }

// info (B) | face_off (B * Fmax) | chunk_tot (B * nch) | start (B * (nch + 1) + 1)
struct Layout {
    size_t info, face, tot, start, total;
};
Layout ws_layout(int Fmax, int B) {
    const size_t nch = (size_t)chunks(Fmax);
    WsBump ws;
    Layout l;
    l.info = ws.put(sizeof(MeshInfo) * (size_t)B);
    l.face = ws.put(sizeof(long long) * (size_t)B * (size_t)Fmax);
    l.tot = ws.put(sizeof(long long) * (size_t)B * nch);
    l.start = ws.put(sizeof(long long) * ((size_t)B * (nch + 1) + 1));
    l.total = ws.at;
    return l;
}

}  // namespace
}  // namespace fx3d

using namespace fx3d;

extern "C" {

fx3d_status fx3d_trimesh_voxel_workspace_bytes(int32_t Vmax, int32_t Fmax, int32_t B, int32_t res, size_t *bytes) {
    FX3D_REQUIRE(bytes && Vmax > 0 && Fmax >= 0 && B > 0 && res > 0 && res <= 1024,
                 "fx3d_trimesh_voxel_workspace_bytes: bad arguments");
    *bytes = ws_layout(Fmax, B).total;
    return FX3D_OK;
}

fx3d_status fx3d_trimesh_to_voxel(const float *verts_padded, int32_t Vmax, const int32_t *verts_len,
                                  const int32_t *faces_padded, int32_t Fmax, const int32_t *faces_len, int32_t B,
                                  int32_t res, float *voxels, uint32_t *bad_dev, void *ws, size_t ws_bytes,
                                  fx3d_stream_t s) {
    FX3D_REQUIRE(verts_padded && verts_len && voxels && ws, "fx3d_trimesh_to_voxel: null pointer");
    FX3D_REQUIRE(Fmax == 0 || (faces_padded && faces_len), "fx3d_trimesh_to_voxel: null faces");
    FX3D_REQUIRE(Vmax > 0 && Vmax <= INT32_MAX / 3 && Fmax >= 0 && B > 0 && res > 0 && res <= 1024 &&
                     (long long)B * (chunks(Fmax) + 1) < INT32_MAX,
                 "fx3d_trimesh_to_voxel: bad sizes");
    FX3D_REQUIRE_GRID_Y("fx3d_trimesh_to_voxel", B, 1);  // (tv_count_kernel; before the memset of `voxels`)
    const Layout l = ws_layout(Fmax, B);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_trimesh_to_voxel: workspace too small");
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    MeshInfo *info = reinterpret_cast<MeshInfo *>(w + l.info);
    long long *face_off = reinterpret_cast<long long *>(w + l.face);
    long long *chunk_tot = reinterpret_cast<long long *>(w + l.tot);
    long long *start = reinterpret_cast<long long *>(w + l.start);
    const int nch = chunks(Fmax);
    const double r = 1.0 / (double)res;
    const double thr = r * r;  // smallest_side = (1.0 / resolution)^2 (:153)
    FX3D_FILL(voxels, 0, sizeof(float) * (size_t)res * res * res * B, st);
    ProfileScope prof("trimesh_to_voxel", st);
    hipLaunchKernelGGL(tv_range_kernel, dim3(B), dim3(kPlanThreads), 0, st, verts_padded, Vmax, verts_len, info, bad_dev);
    if (nch > 0)
        hipLaunchKernelGGL(tv_count_kernel, dim3(nch, B), dim3(kPlanThreads), 0, st, verts_padded, Vmax, verts_len,
                           faces_padded, Fmax, faces_len, thr, info, face_off, chunk_tot, bad_dev);
    hipLaunchKernelGGL(tv_scan_kernel, dim3(1), dim3(kPlanThreads), 0, st, verts_len, Vmax, B, nch, info, chunk_tot, start);
    hipLaunchKernelGGL(tv_slots_kernel, dim3(8 * device_cus()), dim3(kSlotThreads), 0, st, verts_padded, Vmax, verts_len,
                       faces_padded, Fmax, faces_len, B, nch, res, thr, info, face_off, start, voxels);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
