// voxel_to_trimesh with algo :Exact / _voxel_exact (src/conversions.jl:209-232, 246-349) for device-resident grids.
//
// The reference handles every grid b of a (res,res,res,B) Float32 VoxelGrid on its own:
//   1. _assert_voxel (src/rep/voxels.jl:53): every element satisfies 0 <= x <= 1 (NaN fails), else it throws.
//   2. voxel .>= Float32(thresh).
//   3. res >= 3 only: a cell with all three indices in 2:res-1 is cleared when it and its six face neighbours are set.  The
//      right-hand side reads the UN-eroded grid (Julia slicing copies); cells on the grid's outer faces are never cleared.
//   4. Every surviving cell, column-major (first index x fastest), 1-based (x,y,z), appends cube j (0-based, in that order):
//      8 vertices (x-1,y-1,z-1) (x-1,y-1,z) (x-1,y,z-1) (x-1,y,z) (x,y-1,z-1) (x,y-1,z) (x,y,z-1) (x,y,z) -- vertex k takes
//      x-1 + bit 2 of k, y-1 + bit 1, z-1 + bit 0 -- and the 12 faces of cube_faces (kCubeFaces below) plus 8j.
//   5. v ./ maximum(v): one scalar, the largest max(x,y,z) over the survivors; every numerator is an integer in [0, res].
//   6. K = 0 survivors: maximum of an empty array throws.
// Three phases share one bit-packed image: W = ceil(res/64) uint64 words per x row, word r of a grid = w + W*(y + res*z).
//   count  launch 1 (grid-stride, a wave per word)  the Float32 grid read once, 256 contiguous bytes per wave-load; a 64-bit
//                  __ballot of `v >= thresh` is the occupancy word, a ballot of `!(0 <= v <= 1)` counts invalid elements
//                  (one integer atomicAdd per wave-word that has any).
//          launch 2 (one thread per word)  erosion on the bits: x±1 by shifts with the neighbouring words' edge bits, y±1
//                  and z±1 from the words W and W*res away.  Survivor words; per tile (64 words, one wave) its popcount;
//                  per grid an integer atomicMax of max(x,y,z).
//          launch 3 (one block)  int64 exclusive scan of the tile counts over the whole batch (tiles never straddle grids,
//                  so the prefix is the cube's index in the packed vertex array), K per grid into cubes_dev.
//   emit   launch 4 (one block per tile)  the tile's survivors compacted into LDS in rank order, the per-grid quotient table
//                  i / m (i = 0..res, a correctly rounded division) in LDS; then 96 contiguous vertex bytes per cube and
//                  optionally 144 face bytes, both written by the whole block as one contiguous float4 / int4 stream.
//          launch 5 (optional)  zero the padding of faces_padded behind each grid's 12 K faces.
// Cube placement is a prefix sum: no atomics place anything, no float atomics anywhere, bit-identical run to run.
#include "fx3d_common.h"
#include "scan_common.h"

namespace fx3d {
namespace {

constexpr int kThreads = 256;
constexpr int kTileWords = kWave;                 // one wave of words per tile
constexpr int kTileCells = kTileWords * 64;       // survivors per tile at most
constexpr int kScanThreads = 1024;
constexpr int kBinUnroll = 4;                     // words in flight per wave in launch 1
constexpr int kPadBlocks = 16;                    // blocks per grid of the face-padding launch

// cube_faces (src/conversions.jl:313-349), 0-based, 3 bits per entry: entries 0..20 in the low word, 21..35 in the high one
constexpr unsigned char kCubeFaces[36] = {0, 6, 4, 0, 2, 6, 0, 3, 2, 0, 1, 3, 2, 7, 6, 2, 3, 7,
                                          4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 1, 5, 7, 1, 7, 3};
constexpr unsigned long long pack_faces(int from, int to) {
    unsigned long long v = 0;
    for (int i = to - 1; i >= from; --i) v = (v << 3) | kCubeFaces[i];
    return v;
}
constexpr unsigned long long kFacesLo = pack_faces(0, 21), kFacesHi = pack_faces(21, 36);
__device__ __forceinline__ int cube_face(int c) {  // c in [0, 36)
    return (int)((c < 21 ? kFacesLo >> (3 * c) : kFacesHi >> (3 * (c - 21))) & 7ull);
}

struct Dims {
    int res, W, B, tpg;  // tpg: tiles per grid
    long long wpg;       // words per grid = res * res * W
};
Dims dims_of(int res, int B) {
    Dims d;
    d.res = res;
    d.W = (res + 63) / 64;
    d.B = B;
    d.wpg = (long long)res * res * d.W;
    d.tpg = (int)((d.wpg + kTileWords - 1) / kTileWords);
    return d;
}

// launch 1: occupancy words and invalid-element counts.
__global__ __launch_bounds__(kThreads) void vm_binarize_kernel(const float *__restrict__ vox, Dims d, float thresh,
                                                               unsigned long long *__restrict__ occ,
                                                               uint32_t *__restrict__ bad) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long nwords = d.wpg * d.B;
    const long long wave = ((long long)blockIdx.x * kThreads + threadIdx.x) / kWave;
    const long long nwaves = (long long)gridDim.x * (kThreads / kWave);
    const long long rr = (long long)d.res * d.res;
    for (long long g0 = wave * kBinUnroll; g0 < nwords; g0 += nwaves * kBinUnroll) {
        float v[kBinUnroll];
        bool in[kBinUnroll];
#pragma unroll
        for (int u = 0; u < kBinUnroll; ++u) {  // every load first: kBinUnroll x 256 B in flight per wave
            const long long g = g0 + u;
            const long long row = g / d.W;  // b * res^2 + y + res * z
            const int x = (int)(g - row * d.W) * 64 + lane;
            in[u] = g < nwords && x < d.res;
            v[u] = in[u] ? vox[row * d.res + x] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kBinUnroll; ++u) {
            const long long g = g0 + u;
            if (g >= nwords) break;  // wave-uniform
            const unsigned long long set = __ballot(in[u] && v[u] >= thresh);
            const unsigned long long inval = __ballot(in[u] && !(v[u] >= 0.0f && v[u] <= 1.0f));
            if (lane == 0) {
                occ[g] = set;
                if (inval) atomicAdd(bad + (g / d.W) / rr, (uint32_t)__popcll(inval));
            }
        }
    }
}

// bits x in [1, res-2] of word w (the cells erosion may clear along x)
__device__ __forceinline__ unsigned long long interior_x(int w, int res) {
    const int lo = max(1 - 64 * w, 0), hi = min(res - 2 - 64 * w, 63);
    if (lo > hi) return 0ull;
    const unsigned long long upto = hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1);
    return upto & ~((1ull << lo) - 1);
}

// launch 2: block = 4 tiles of one grid (a wave per tile, a lane per word).
__global__ __launch_bounds__(kThreads) void vm_erode_kernel(const unsigned long long *__restrict__ occ, Dims d,
                                                            unsigned long long *__restrict__ surv,
                                                            int32_t *__restrict__ tile_cnt, int32_t *__restrict__ gmax) {
    const int bpg = (d.tpg + kThreads / kWave - 1) / (kThreads / kWave);
    const int b = blockIdx.x / bpg;
    const int t = (blockIdx.x % bpg) * (kThreads / kWave) + threadIdx.x / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const long long r = (long long)t * kTileWords + lane;
    const int res = d.res, W = d.W;
    const unsigned long long *base = occ + (size_t)b * d.wpg;
    unsigned long long s = 0;
    int mx = 0;
    if (t < d.tpg && r < d.wpg) {
        unsigned long long cur = base[r];
        const long long row = r / W;
        const int w = (int)(r - row * W), y = (int)(row % res), z = (int)(row / res);
        if (res >= 3 && cur && y >= 1 && y <= res - 2 && z >= 1 && z <= res - 2) {
            const unsigned long long prev = w > 0 ? base[r - 1] : 0ull, next = w < W - 1 ? base[r + 1] : 0ull;
            const unsigned long long xm = (cur << 1) | (prev >> 63), xp = (cur >> 1) | (next << 63);
            const long long zs = (long long)W * res;
            const unsigned long long all = cur & xm & xp & base[r - W] & base[r + W] & base[r - zs] & base[r + zs];
            cur &= ~(all & interior_x(w, res));
        }
        s = cur;
        surv[(size_t)b * d.wpg + r] = s;
        if (s) mx = max(max(64 * w + 63 - __clzll(s), y), z) + 1;  // max(x, y, z), 1-based
    }
    int cnt = __popcll(s);
    for (int o = kWave / 2; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, kWave);
        mx = max(mx, __shfl_xor(mx, o, kWave));
    }
    if (lane == 0 && t < d.tpg) {
        tile_cnt[(size_t)b * d.tpg + t] = cnt;
        if (mx) atomicMax(gmax + b, mx);
    }
}

// launch 3 (one block): start[i] = survivors in tiles [0, i) of the batch, start[n] = the total; cubes[b] = K of grid b.
__global__ __launch_bounds__(kScanThreads) void vm_scan_kernel(const int32_t *__restrict__ tile_cnt, Dims d,
                                                               long long *__restrict__ start, int64_t *__restrict__ cubes) {
    __shared__ long long sw[kScanThreads / kWave], stot;
    const long long n = (long long)d.tpg * d.B;
    long long carry = 0;
    for (long long base = 0; base < n; base += kScanThreads) {
        const long long e = base + threadIdx.x;
        const long long ex = block_exclusive_scan_serial(e < n ? tile_cnt[e] : 0, sw, &stot);
        if (e < n) start[e] = carry + ex;
        carry += stot;
    }
    if (threadIdx.x == 0) start[n] = carry;
    __syncthreads();
    for (int b = threadIdx.x; b < d.B; b += kScanThreads)
        cubes[b] = start[(long long)(b + 1) * d.tpg] - start[(long long)b * d.tpg];
}

// launch 4: block = one tile.  Vertices at 24 * (global cube index) floats; faces at grid b's column block, mesh-local.
__global__ __launch_bounds__(kThreads) void vm_emit_kernel(const unsigned long long *__restrict__ surv, Dims d,
                                                           const long long *__restrict__ start,
                                                           const int32_t *__restrict__ gmax, long long max_cubes,
                                                           float *__restrict__ verts, int32_t *__restrict__ faces, int Fmax) {
    __shared__ uint32_t cells[kTileCells];  // x | y << 10 | z << 20, 0-based, in rank order
    __shared__ float quot[1025];
    const long long tile = blockIdx.x;
    const int b = (int)(tile / d.tpg), t = (int)(tile % d.tpg);
    const long long s0 = start[tile];
    const int cnt = (int)(start[tile + 1] - s0);
    if (cnt == 0 || s0 + cnt > max_cubes) return;  // (block-uniform) nothing here, or beyond the caller's capacity
    const long long g0 = start[(long long)b * d.tpg];
    const long long K = start[(long long)(b + 1) * d.tpg] - g0;
    const long long j0 = s0 - g0;  // mesh-local index of the tile's first cube
    const float m = (float)gmax[b];
    for (int i = threadIdx.x; i <= d.res; i += kThreads) quot[i] = (float)i / m;  // v ./ maximum(v): a true division
    if (threadIdx.x < kWave) {
        const int lane = threadIdx.x;
        const long long r = (long long)t * kTileWords + lane;
        unsigned long long s = r < d.wpg ? surv[(size_t)b * d.wpg + r] : 0ull;
        const int pc = __popcll(s);
        int inc = pc;
        for (int o = 1; o < kWave; o <<= 1) {
            const int u = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += u;
        }
        int pos = inc - pc;
        const long long row = r / d.W;
        const uint32_t yz = ((uint32_t)(row % d.res) << 10) | ((uint32_t)(row / d.res) << 20);
        const int x0 = (int)(r - row * d.W) * 64;
        while (s) {
            cells[pos++] = yz | (uint32_t)(x0 + __ffsll((long long)s) - 1);
            s &= s - 1;
        }
    }
    __syncthreads();
    float4 *vo = reinterpret_cast<float4 *>(verts + 24 * s0);  // 96 B per cube: 16-byte aligned
    for (int u = threadIdx.x; u < 6 * cnt; u += kThreads) {
        const int q = u / 6, p = u - 6 * q;
        const uint32_t cell = cells[q];
        const int cx = (int)(cell & 1023u), cy = (int)((cell >> 10) & 1023u), cz = (int)(cell >> 20);
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * p + i, k = c / 3, a = c - 3 * k;  // vertex k, axis a: x-1 + bit 2, y-1 + bit 1, z-1 + bit 0
            e[i] = quot[(a == 0 ? cx : a == 1 ? cy : cz) + ((k >> (2 - a)) & 1)];
        }
        vo[u] = make_float4(e[0], e[1], e[2], e[3]);
    }
    if (!faces || 12 * K > (long long)Fmax) return;
    int32_t *fo = faces + (size_t)b * 3 * Fmax + 36 * j0;
    const int base = (int)(8 * j0);
    if ((Fmax & 3) == 0) {  // 144 B per cube and a 16-byte aligned column block
        int4 *f4 = reinterpret_cast<int4 *>(fo);
        for (int u = threadIdx.x; u < 9 * cnt; u += kThreads) {
            const int q = u / 9, c = 4 * (u - 9 * q), o = base + 8 * q;
            f4[u] = make_int4(cube_face(c) + o, cube_face(c + 1) + o, cube_face(c + 2) + o, cube_face(c + 3) + o);
        }
    } else {
        for (int u = threadIdx.x; u < 36 * cnt; u += kThreads) {
            const int q = u / 36;
            fo[u] = cube_face(u - 36 * q) + base + 8 * q;
        }
    }
}

// launch 5: faces_padded entries behind grid b's 12 K faces are 0 (the library's pad value, like index_upload's)
__global__ __launch_bounds__(kThreads) void vm_face_pad_kernel(const long long *__restrict__ start, Dims d,
                                                               int32_t *__restrict__ faces, int Fmax) {
    const int b = blockIdx.x / kPadBlocks, sub = blockIdx.x % kPadBlocks;
    const long long K = start[(long long)(b + 1) * d.tpg] - start[(long long)b * d.tpg];
    if (12 * K > (long long)Fmax) return;
    int32_t *fb = faces + (size_t)b * 3 * Fmax;
    for (long long e = 36 * K + (long long)sub * kThreads + threadIdx.x; e < 3ll * Fmax; e += (long long)kPadBlocks * kThreads)
        fb[e] = 0;
}

// occ (B * wpg u64) | surv (B * wpg u64) | tile_cnt (B * tpg i32) | start (B * tpg + 1 i64) | gmax (B i32)
struct Layout {
    size_t occ, surv, cnt, start, gmax, total;
};
Layout layout(const Dims &d) {
    const size_t words = (size_t)d.wpg * d.B, tiles = (size_t)d.tpg * d.B;
    WsBump ws;
    Layout l;
    l.occ = ws.put(8 * words);
    l.surv = ws.put(8 * words);
    l.cnt = ws.put(4 * tiles);
    l.start = ws.put(8 * (tiles + 1));
    l.gmax = ws.put(4 * (size_t)d.B);
    l.total = ws.at;
    return l;
}

bool sizes_ok(int32_t res, int32_t B) {
    return res >= 1 && res <= 1024 && B >= 1 && B <= (1 << 24) && (long long)dims_of(res, B).tpg * B < INT32_MAX;
}

}  // namespace
}  // namespace fx3d

using namespace fx3d;

extern "C" {

fx3d_status fx3d_voxel_mesh_workspace_bytes(int32_t res, int32_t B, size_t *bytes) {
    FX3D_REQUIRE(bytes && sizes_ok(res, B), "fx3d_voxel_mesh_workspace_bytes: bad arguments");
    *bytes = layout(dims_of(res, B)).total;
    return FX3D_OK;
}

fx3d_status fx3d_voxel_mesh_count(const float *voxels, int32_t res, int32_t B, float thresh, int64_t *cubes_dev,
                                  uint32_t *bad_dev, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(voxels && cubes_dev && bad_dev && ws, "fx3d_voxel_mesh_count: null pointer");
    FX3D_REQUIRE(sizes_ok(res, B), "fx3d_voxel_mesh_count: bad sizes");
    const Dims d = dims_of(res, B);
    const Layout l = layout(d);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_voxel_mesh_count: workspace too small");
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    auto *occ = reinterpret_cast<unsigned long long *>(w + l.occ);
    auto *surv = reinterpret_cast<unsigned long long *>(w + l.surv);
    auto *cnt = reinterpret_cast<int32_t *>(w + l.cnt);
    auto *start = reinterpret_cast<long long *>(w + l.start);
    auto *gmax = reinterpret_cast<int32_t *>(w + l.gmax);
    FX3D_FILL(bad_dev, 0, sizeof(uint32_t) * (size_t)B, st);
    FX3D_FILL(gmax, 0, sizeof(int32_t) * (size_t)B, st);
    const long long words = d.wpg * B;
    const long long want = (words + kBinUnroll * (kThreads / kWave) - 1) / (kBinUnroll * (kThreads / kWave));
    const int bin_blocks = (int)(want < 8ll * device_cus() ? want : 8ll * device_cus());
    const int bpg = (d.tpg + kThreads / kWave - 1) / (kThreads / kWave);
    ProfileScope prof("voxel_mesh_count", st);
    hipLaunchKernelGGL(vm_binarize_kernel, dim3(bin_blocks), dim3(kThreads), 0, st, voxels, d, thresh, occ, bad_dev);
    hipLaunchKernelGGL(vm_erode_kernel, dim3((unsigned)((long long)bpg * B)), dim3(kThreads), 0, st, occ, d, surv, cnt, gmax);
    hipLaunchKernelGGL(vm_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, cnt, d, start, cubes_dev);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_voxel_mesh_emit(int32_t res, int32_t B, int64_t max_cubes, float *verts_packed, int32_t *faces_padded,
                                 int32_t Fmax, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(ws && (verts_packed || max_cubes == 0), "fx3d_voxel_mesh_emit: null pointer");
    FX3D_REQUIRE(sizes_ok(res, B) && max_cubes >= 0 && (!faces_padded || Fmax > 0), "fx3d_voxel_mesh_emit: bad sizes");
    const Dims d = dims_of(res, B);
    const Layout l = layout(d);
    FX3D_REQUIRE(ws_bytes >= l.total, "fx3d_voxel_mesh_emit: workspace too small");
    hipStream_t st = as_stream(s);
    char *w = static_cast<char *>(ws);
    auto *surv = reinterpret_cast<const unsigned long long *>(w + l.surv);
    auto *start = reinterpret_cast<const long long *>(w + l.start);
    auto *gmax = reinterpret_cast<const int32_t *>(w + l.gmax);
    ProfileScope prof("voxel_mesh_emit", st);
    hipLaunchKernelGGL(vm_emit_kernel, dim3((unsigned)((long long)d.tpg * B)), dim3(kThreads), 0, st, surv, d, start, gmax,
                       (long long)max_cubes, verts_packed, faces_padded, Fmax);
    if (faces_padded)
        hipLaunchKernelGGL(vm_face_pad_kernel, dim3((unsigned)(B * kPadBlocks)), dim3(kThreads), 0, st, start, d,
                           faces_padded, Fmax);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
