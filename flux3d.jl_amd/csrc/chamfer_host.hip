// Chamfer forward / nearest neighbours, the host path: the launch plan and its cost model, the workspace layout, the drivers,
// the kernels that turn sums into the loss, and the C entry points.  The nearest-neighbour kernels are in chamfer.hip (fp16
// filter, D = 3) and nn1_exact.hip (the exact loops); nn1_common.h holds what the three units share.
#include <cmath>
#include <cstdlib>

#include "nn1_common.h"

using namespace fx3d;

namespace {

// Fixed-order reduction of the per-block partials into sums[0..1] (+ optional loss).
struct FinalizeParams {
    const double *partials;
    int B, tiles, tiles_x, tiles_y;
    double *sums;  // [2]
    // optional loss (loss != nullptr)
    float *loss;
    int N, M, D;
    long long Bg;
    float w1, w2;
};

__global__ __launch_bounds__(kThreads) void chamfer_finalize_partials_kernel(FinalizeParams f) {
    __shared__ double sm[kThreads / 64];
    double tot[2];
    for (int dir = 0; dir < 2; ++dir) {
        const int nt = dir ? f.tiles_y : f.tiles_x;
        const long long n = (long long)f.B * nt;
        double acc = 0.0;
        for (long long k = threadIdx.x; k < n; k += kThreads) {
            const int b = (int)(k / nt), t = (int)(k % nt);
            acc += f.partials[((size_t)(dir * f.B + b)) * f.tiles + t];
        }
        __syncthreads();
        tot[dir] = block_sum<kThreads>(acc, sm);
    }
    if (threadIdx.x == 0) {
        if (f.sums) { f.sums[0] = tot[0]; f.sums[1] = tot[1]; }
        if (f.loss) *f.loss = chamfer_loss_from_sums(tot[0], tot[1], f.N, f.M, f.D, f.Bg, f.w1, f.w2);
    }
}

__global__ void chamfer_loss_kernel(const double *sums, int N, int M, int D, long long Bg,
                                    float w1, float w2, float *loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        *loss = chamfer_loss_from_sums(sums[0], sums[1], N, M, D, Bg, w1, w2);
}

__global__ void chamfer_loss_many_kernel(const double *sums, int count, int N, int M, int D, long long Bg,
                                         float w1, float w2, float *loss) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) loss[i] = chamfer_loss_from_sums(sums[2 * i], sums[2 * i + 1], N, M, D, Bg, w1, w2);
}

struct Plan {
    int R, tiles_x, tiles_y, tiles, chunk, grid;
    size_t lds_bytes;
    int variant;  // 0 = exact hot loop (D = 2, and D = 3 under FX3D_NN1_VARIANT=0), 3 = fp16-split MFMA filter + exact re-scan,
                  // 4 = nn1_tiny_kernel (D = 3, small problems: exact, no per-cloud statistics / image)
    int threads, tpb, tpb_y;  // tpb: passes per block of the x -> y direction, tpb_y: of y -> x
    int nsplit;  // fp16 variant: chunk subsets per query tile (multi-chunk clouds with too few blocks)
    int tail;    // fp16 variant: kHTail when clouds of chunk + (1 .. kHTail) points run as one chunk + an exact tail
};

// option nn1_variant = 0 selects the exact VALU loop for D = 3 (A/B measurements; the f32 VALU / MFMA filter variants
// of round 1 are in the history: DESIGN.md 3.1 "ladder").
int nn1_variant() { return opt(OPT_NN1_VARIANT) == 0 ? 0 : 3; }

// nn1_f16_kernel's cost model, in microseconds, measured at C2 (tools/nn1_probe.hip): bounding box per 4096 candidates of the
// cloud, image per 4096 of the chunk + a constant per chunk, one pass (filter + exact) per 4096 + a constant per pass.
constexpr double kUsBox = 2.8, kUsImage = 5.0, kUsChunk = 0.5, kUsPass = 9.7, kUsPassFixed = 0.8;
// A block's time: the box of its cloud of `nc` candidates, then `nchunks` images of `ch` candidates with `tpb` passes over each.
// (The plans compare sums of these with a margin of 1e-9: every unit cost is a multiple of 0.1 / 4096, so two plans' times are
// equal or at least ~1e-7 apart once divided by the CU count, and the order of the additions cannot change a choice.)
double block_us(int nc, int ch, int nchunks, int tpb) {
    const double per_chunk = kUsImage * ch / 4096.0 + kUsChunk + tpb * (kUsPass * ch / 4096.0 + kUsPassFixed);
    return kUsBox * nc / 4096.0 + nchunks * per_chunk;
}
int ceil_div(int n, int d) { return (n + d - 1) / d; }

Plan make_plan(int N, int M, int B, int D, bool allow_split = true) {
    Plan pl{};
    const long long work = (long long)B * ((long long)N + M);  // total queries, both directions
    pl.variant = D == 3 ? nn1_variant() : 0;
    pl.threads = pl.variant == 3 ? kHThreads : kThreads;
    // exact loop: R queries per thread -- enough blocks to fill 256 CUs x ~2 blocks, but as much register
    // blocking (LDS-read amortisation, ILP) as the problem size allows.
    int R = 4;
    while (R > 1 && work / (kThreads * R) < 512) R >>= 1;
    pl.R = R;
    pl.tpb = pl.tpb_y = 1;
    const int maxc0 = N > M ? N : M;
    const int clouds8 = (2 * B + 7) / 8;
    pl.nsplit = 1;
    if (D != 2 && D != 3) {
        // nn1_generic_kernel: one query per thread, 256-query tiles, no LDS staging
        pl.R = 1;
        pl.tiles_x = (N + kThreads - 1) / kThreads;
        pl.tiles_y = (M + kThreads - 1) / kThreads;
        pl.tiles = pl.tiles_x > pl.tiles_y ? pl.tiles_x : pl.tiles_y;
        pl.chunk = 0;
        pl.lds_bytes = 0;
        pl.grid = 2 * B * pl.tiles;  // (< 2^30: chamfer_check_shapes)
        return pl;
    }
    if (pl.variant == 3 && 2ll * B * (long long)N * M <= 1000000ll * opt(OPT_NN1_TINY_MPAIRS)) {
        // small problem: the exact kernel without statistics / image (C1, the reference harness's n <= 1024).  Two queries per
        // lane once 16-query blocks would be more than two rounds of the chip
        pl.variant = 4;
        pl.threads = kTyThreads;
        const int cus = device_cus();
        pl.R = work / kTyQ > 2ll * cus ? 2 : 1;
        const int per = kTyQ * pl.R;
        const int rx = (N + per - 1) / per, ry = (M + per - 1) / per;   // query tiles per cloud and direction
        int tpb = 1;                                                     // consecutive tiles per block: at most ~2 blocks per CU
        while ((long long)B * ((rx + tpb - 1) / tpb + (ry + tpb - 1) / tpb) > 2ll * cus && tpb < (rx > ry ? rx : ry)) tpb *= 2;
        pl.tpb = pl.tpb_y = tpb;
        pl.tiles_x = (rx + tpb - 1) / tpb;
        pl.tiles_y = (ry + tpb - 1) / tpb;
        pl.tiles = pl.tiles_x > pl.tiles_y ? pl.tiles_x : pl.tiles_y;
        pl.chunk = 0;
        pl.lds_bytes = 0;
        pl.grid = 2 * B * pl.tiles;
        return pl;
    }
    if (pl.variant == 0) {
        const int per_block = kThreads * R;
        pl.tiles_x = (N + per_block - 1) / per_block;
        pl.tiles_y = (M + per_block - 1) / per_block;
        pl.tiles = pl.tiles_x > pl.tiles_y ? pl.tiles_x : pl.tiles_y;
        int chunk = (maxc0 + kTile - 1) / kTile * kTile;
        if (chunk > kChunkMax) chunk = kChunkMax;
        pl.chunk = chunk;
        pl.lds_bytes = (size_t)chunk * D * sizeof(float);
        pl.grid = clouds8 * 8 * pl.tiles;
        return pl;
    }
    // nn1_f16_kernel: choose (candidate chunk size, chunks per block, 512-query passes per block) by the cost
    // model above (block_us) and the blocks resident at once (one per CU).
    // A block either walks all chunks serially (one pass per block: the per-query slot lives in LDS) or takes
    // ONE chunk of a split run (any number of passes; the subsets' rows merge in the same launch since round 5).  A split
    // plan is charged 8 us: no longer a second launch, a FITTED constant -- swept 8 / 5 / 3 over tools/nn1_shapes_time.py's
    // shapes on one box, only 8 x 8192 x 8192 changes plan, and the lower charges pick the slower one (62 us against 55.5:
    // the model under-prices 2048-candidate images run four passes each).  Few large clouds want many small chunks, many
    // small clouds want passes.
    const int cmax = kHChunkMax, gran = 32 * kHLT;
    const int ncu = device_cus();  // blocks resident at once: one per CU (256 on an MI355X in SPX mode)
    // a larger cloud of at most cmax + kHTail points is planned (and run) as ONE chunk of cmax with an exact tail
    int maxc = maxc0, b_chunk = 0, b_tpb = 1, b_split = 1;
    auto search = [&](int mc) {  // mc: the candidates that go through LDS images
        maxc = mc;
        const int cminc = (maxc + cmax - 1) / cmax;
        double best = 1e30;
        b_chunk = (maxc + gran - 1) / gran * gran < cmax ? (maxc + gran - 1) / gran * gran : cmax; b_tpb = 1; b_split = 1;
        for (int nch = cminc; nch <= cminc * 8 && nch <= 64; ++nch) {
            int ch = ((maxc + nch - 1) / nch + gran - 1) / gran * gran;
            if (ch > cmax) continue;
            const int anch = (maxc + ch - 1) / ch;
            for (int split = 0; split < 2; ++split) {
                if (split && (!allow_split || anch == 1 || opt(OPT_NN1_NOSPLIT))) continue;
                for (int tpb = 1; tpb <= 8; tpb *= 2) {
                    if (!split && anch > 1 && tpb > 1) continue;
                    const long long tiles = ceil_div(maxc, 512 * tpb);
                    const long long blocks = 2ll * B * tiles * (split ? anch : 1);
                    const double t_block = block_us(maxc, ch, split ? 1 : anch, tpb);
                    const double rounds = (double)((blocks + ncu - 1) / ncu);
                    const double t = rounds * t_block + (split ? 8.0 : 0.0);
                    if (t < best - 1e-9) { best = t; b_chunk = ch; b_tpb = tpb; b_split = split ? anch : 1; }
                }
            }
        }
    };
    // a cloud of cmax + (1 .. kHTail) points: planned as cmax; kept if that plan is ONE chunk of cmax per block (then the kernel
    // runs the tail exactly), otherwise planned again at its true size
    pl.tail = 0;
    if (maxc0 > cmax && maxc0 - cmax <= kHTail) {
        search(cmax);
        if (b_split == 1 && b_chunk == cmax) pl.tail = kHTail;
    }
    if (!pl.tail) search(maxc0);
    pl.chunk = b_chunk;
    pl.tpb = pl.tpb_y = b_tpb;
    pl.nsplit = b_split;
    pl.lds_bytes = nn1_f16_lds_bytes(pl.chunk);
    if (N != M && b_split == 1 && maxc <= b_chunk) {
        // clouds of different sizes, one chunk each: the direction whose CANDIDATES are the large cloud has few, heavy blocks
        // (N = 4096 against M = 1024 at B = 32: 32 blocks as long as C2's on 32 CUs while the rest of the chip idles) -- the
        // passes per block are chosen per direction: t = the slower direction's block, or the chip's throughput if the
        // blocks of both do not fit at once
        double bt = 1e30;
        for (int ta = 1; ta <= 8; ta *= 2)
            for (int tb = 1; tb <= 8; tb *= 2) {
                const double blk_a = block_us(M, M, 1, ta);  // x -> y: candidates y
                const double blk_b = block_us(N, N, 1, tb);  // y -> x: candidates x
                const int tiles_a = ceil_div(N, 512 * ta), tiles_b = ceil_div(M, 512 * tb);
                const double na = (double)B * tiles_a, nb = (double)B * tiles_b;
                const double thr = (na * blk_a + nb * blk_b) / (double)ncu;
                double t = blk_a > blk_b ? blk_a : blk_b;
                t = t > thr ? t : thr;
                // the grid has max(tiles) slots per (cloud, direction): more than one round of them delays the heavy direction's blocks
                const long long tmax = tiles_a > tiles_b ? tiles_a : tiles_b;
                t += 1.0 * (double)((2ll * B * tmax + ncu - 1) / ncu - 1);
                if (t < bt - 1e-9) { bt = t; pl.tpb = ta; pl.tpb_y = tb; }
            }
    }
    // one-chunk plans: a remainder of <= kHTail queries beyond a direction's last full tile is one more pass of that tile's block
    // (one wave busy for ~6 us) instead of a block of its own (prologue + a pass: a second round of blocks at N = 4097)
    const bool fold = b_split == 1 && maxc <= b_chunk;
    auto ntiles = [&](int nq, int tpb) {
        const int per = 512 * tpb;
        int t = ceil_div(nq, per);
        if (fold && t > 1 && nq - (t - 1) * per <= kHTail) --t;
        return t;
    };
    pl.tiles_x = ntiles(N, pl.tpb);
    pl.tiles_y = ntiles(M, pl.tpb_y);
    pl.tiles = pl.tiles_x > pl.tiles_y ? pl.tiles_x : pl.tiles_y;
    pl.grid = clouds8 * 8 * pl.tiles * pl.nsplit;
    if (2 * B < 8) pl.grid = 2 * B * pl.tiles * pl.nsplit;  // plain block order (see kernel)
    return pl;
}

// the kernel a plan launches: read by fx3d_nn1_plan_describe, the drivers and the pruning rule
Nn1Kernel plan_kernel(const Plan &pl, int D) {
    if (D != 2 && D != 3) return NN1_GENERIC;
    return pl.variant == 3 ? NN1_F16 : pl.variant == 4 ? NN1_TINY : NN1_SMALL_D;
}
const char *plan_kernel_name(const Plan &pl, int D) {
    static const char *const names[] = {"generic", "small_d", "tiny", "f16"};  // (by Nn1Kernel)
    return names[plan_kernel(pl, D)];
}

// Spatial pruning (nn1_f16_kernel<.., PRUNE>): one-chunk plans of the fp16 kernel without split or tail, clouds of at least 1024
// points.  Slots of scratch per block (a 16-bit original index each): the candidate cloud in image order + the block's window of
// the query cloud.
int prune_rows_per_block(const Plan &pl, int N, int M, int D) {
    const int maxc = N > M ? N : M;
    if (plan_kernel(pl, D) != NN1_F16 || pl.nsplit != 1 || pl.tail != 0 || maxc > pl.chunk || maxc < 1024 || !opt(OPT_NN1_PRUNE)) return 0;
    // one pass per block does not repay the sort (measured at B = 8 .. 16 x 4096: 36 against 30 us; two passes -- C2 -- 46 against 53)
    if ((pl.tpb < pl.tpb_y ? pl.tpb : pl.tpb_y) < 2) return 0;
    return kHScrCand + (pl.tpb > pl.tpb_y ? pl.tpb : pl.tpb_y) * 512 + kHTail;
}

// The caller's workspace, as byte offsets: the per-block partial sums at 0 (`tiles` per (direction, cloud): the plan's, or the
// 256-query tiles of a split run's unpack kernel), two doubles for the sums behind them, a split run's per-query merge rows, and --
// rounded up to 256 bytes -- the pruning scratch.  `need` is the size below which a call fails; a workspace of at least `total`
// (what fx3d_chamfer_workspace_bytes answers) also holds the scratch, a smaller one runs without pruning.
struct Workspace {
    int tiles;
    size_t sums, gres, need, pscr, total;
};
Workspace workspace_layout(const Plan &pl, int N, int M, int B, int D) {
    Workspace w{};
    const int maxq = N > M ? N : M;
    w.tiles = pl.nsplit > 1 ? ceil_div(maxq, kThreads) : pl.tiles;
    w.sums = (size_t)2 * B * w.tiles * sizeof(double);
    w.gres = w.sums + 2 * sizeof(double);
    w.need = w.gres + (pl.nsplit > 1 ? (size_t)pl.nsplit * 2 * B * maxq * sizeof(unsigned long long) : 0);
    w.pscr = (w.need + 255) & ~(size_t)255;
    const size_t ps = (size_t)prune_rows_per_block(pl, N, M, D) * pl.grid * sizeof(unsigned short);
    w.total = ps ? w.pscr + ps : w.need;
    return w;
}

constexpr long long kSplitFuseMax = 255;  // tile counters of a fused split run: the 15 spare words of each of a ticket slot's 17 lines

// One nearest-neighbour launch.  The caller says WHAT (`p`: inputs, outputs, partials, the fused finalisation's ticket and
// outputs, a split run's rows, pruning scratch); how -- the plan's geometry and what follows from it -- is filled in here.
fx3d_status run_nn1(Nn1Params p, int D, const Plan &pl, hipStream_t st) {
    p.tiles = pl.tiles; p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.chunk = pl.chunk;
    p.tpb = pl.tpb; p.tpb_y = pl.tpb_y;
    p.tail = pl.tail;
    p.nsplit = p.gres ? pl.nsplit : 1;
    p.fuse_split = p.gres && p.ticket ? 1 : 0;  // (the caller checked that the tile counters fit the ticket slot)
    p.pscr_stride = p.pscr ? prune_rows_per_block(pl, p.N, p.M, D) : 0;
    if (!p.pscr_stride) p.pscr = nullptr;
    // The pruned instantiation has these as compile-time facts (chamfer.hip: one chunk holds each candidate cloud, no candidate split, no
    // tail, no split rows): a plan that breaks one must not reach it.
    if (p.pscr)
        FX3D_REQUIRE(p.nsplit == 1 && p.tail == 0 && !p.gres && (p.N > p.M ? p.N : p.M) <= p.chunk && p.chunk <= kHChunkMax,
                     "nn1: pruning scratch with a plan the pruned kernel does not take (nsplit=%d tail=%d chunk=%d N=%d M=%d)", p.nsplit, p.tail,
                     p.chunk, p.N, p.M);
    const Nn1Kernel k = plan_kernel(pl, D);
    ProfileScope prof("nn1", st);
    if (k == NN1_F16) return nn1_f16_launch(p, pl.grid, pl.lds_bytes, st);
    return nn1_exact_launch(k, p, D, pl.R, pl.grid, pl.lds_bytes, st);
}

}  // namespace

namespace fx3d {

fx3d_status chamfer_check_shapes(const char *fn, const void *x, int N, const void *y, int M, int B, int D) {
    FX3D_REQUIRE(x && y, "%s: null input pointer", fn);
    FX3D_REQUIRE(N > 0 && M > 0 && B > 0 && D > 0, "%s: empty input (N=%d M=%d B=%d D=%d)", fn, N, M, B, D);
    FX3D_REQUIRE((long long)B * 2 * (((long long)(N > M ? N : M) + 255) / 256) < (1ll << 30),
                 "%s: problem too large for one launch", fn);
    return FX3D_OK;
}

// The forward driver: the two sums (sums_dev) and / or the loss with batch size Bg (loss_dev), optional indices.
fx3d_status chamfer_forward(const float *x, int N, const float *y, int M, int B, int D, double *sums_dev, float *loss_dev,
                            long long Bg, float w1, float w2, int32_t *idx_x, int32_t *idx_y, void *ws, size_t ws_bytes,
                            hipStream_t st, const char *fn) {
    fx3d_status rc = chamfer_check_shapes(fn, x, N, y, M, B, D);
    if (rc) return rc;
    const Plan pl = make_plan(N, M, B, D);
    const Workspace w = workspace_layout(pl, N, M, B, D);
    if (!ws || ws_bytes < w.need) {
        set_error("%s: workspace too small (%zu < %zu bytes)", fn, ws ? ws_bytes : (size_t)0, w.need);
        return FX3D_ERR_WORKSPACE;
    }
    // the split plan's two-launch form ends in nn1_split_finalize_launch, whose grid holds both directions of every cloud in y
    if (pl.nsplit > 1 && 2ll * B * pl.tiles > kSplitFuseMax) FX3D_REQUIRE_GRID_Y(fn, B, 2);
    char *const base = static_cast<char *>(ws);
    Nn1Params p{};
    p.x = x; p.y = y; p.N = N; p.M = M; p.B = B;
    p.idx_x = idx_x; p.idx_y = idx_y;
    p.partials = reinterpret_cast<double *>(base);
    p.sums_out = sums_dev ? sums_dev : reinterpret_cast<double *>(base + w.sums);
    p.loss_out = loss_dev; p.w1 = w1; p.w2 = w2; p.Bg = Bg;
    const Nn1Kernel k = plan_kernel(pl, D);
    if (k == NN1_F16 || k == NN1_TINY) {  // the last block to arrive reduces the partials: no finalize launch
        p.ticket = ticket_slot(&rc, st);
        if (!p.ticket) return rc;
        p.nvalid = (unsigned int)((long long)B * pl.tiles_x + (long long)B * pl.tiles_y);
    }
    if (pl.nsplit > 1) {
        // few large clouds (D == 3, fp16 kernel): chunk subsets run in parallel blocks, each stores its per-query result row in
        // gres (plain stores: no memset node, no atomics)
        p.gres = reinterpret_cast<unsigned long long *>(base + w.gres);
        p.qstride = N > M ? N : M;
        // one launch: the last chunk subset of every query tile merges (tile counters in the ticket slot's spare words), the
        // last of those blocks reduces the partials (layout of the one-chunk path: pl.tiles entries per (direction, cloud))
        if (2ll * B * pl.tiles <= kSplitFuseMax) return run_nn1(p, D, pl, st);
        // two launches: the rows alone, then the unpack kernel merges them, writes the outputs and its 256-query tiles' partials
        Nn1Params rows = p;
        rows.idx_x = rows.idx_y = nullptr; rows.partials = nullptr; rows.ticket = nullptr;
        rc = run_nn1(rows, D, pl, st);
        if (rc) return rc;
        p.nsplit = pl.nsplit; p.chunk = pl.chunk;
        p.nvalid = (unsigned int)((long long)w.tiles * 2 * B);
        p.tiles_x = ceil_div(N, kThreads); p.tiles_y = ceil_div(M, kThreads);
        return nn1_split_finalize_launch(p, w.tiles, st);
    }
    // spatial pruning when the workspace holds the blocks' scratch behind the partial sums (fx3d_chamfer_workspace_bytes asks for it)
    if (w.total > w.need && ws_bytes >= w.total) p.pscr = reinterpret_cast<unsigned short *>(base + w.pscr);
    rc = run_nn1(p, D, pl, st);
    if (rc || p.ticket) return rc;
    const FinalizeParams f{p.partials, B, pl.tiles, pl.tiles_x, pl.tiles_y, p.sums_out, loss_dev, N, M, D, Bg, w1, w2};
    hipLaunchKernelGGL(chamfer_finalize_partials_kernel, dim3(1), dim3(kThreads), 0, st, f);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace fx3d

extern "C" {

fx3d_status fx3d_nn1(const float *x, int32_t N, const float *y, int32_t M, int32_t B, int32_t D,
                     int32_t *idx_x, int32_t *idx_y, float *dmin_x, float *dmin_y,
                     fx3d_stream_t s) {
    fx3d_status rc = chamfer_check_shapes("fx3d_nn1", x, N, y, M, B, D);
    if (rc) return rc;
    Plan pl = make_plan(N, M, B, D);
    if (pl.nsplit > 1) {  // no scratch at this entry point: plan without the split option
        pl = make_plan(N, M, B, D, false);
    }
    Nn1Params p{};
    p.x = x; p.y = y; p.N = N; p.M = M; p.B = B;
    p.idx_x = idx_x; p.idx_y = idx_y; p.dmin_x = dmin_x; p.dmin_y = dmin_y;
    return run_nn1(p, D, pl, as_stream(s));
}

fx3d_status fx3d_nn1_plan_describe(int32_t N, int32_t M, int32_t B, int32_t D, char *buf, size_t n) {
    FX3D_REQUIRE(buf && n > 0, "fx3d_nn1_plan_describe: null buffer");
    FX3D_REQUIRE(N > 0 && M > 0 && B > 0 && D > 0, "fx3d_nn1_plan_describe: empty problem");
    const Plan pl = make_plan(N, M, B, D);
    snprintf(buf, n, "variant=%d threads=%d chunk=%d nsplit=%d tpb=%d tpb_y=%d tiles_x=%d tiles_y=%d grid=%d tail=%d lds=%zu R=%d kernel=%s",
             pl.variant, pl.threads, pl.chunk, pl.nsplit, pl.tpb, pl.tpb_y, pl.tiles_x, pl.tiles_y, pl.grid, pl.tail, pl.lds_bytes, pl.R,
             plan_kernel_name(pl, D));
    return FX3D_OK;
}

fx3d_status fx3d_chamfer_workspace_bytes(int32_t N, int32_t M, int32_t B, int32_t D, size_t *bytes) {
    FX3D_REQUIRE(bytes, "fx3d_chamfer_workspace_bytes: null output");
    FX3D_REQUIRE(N > 0 && M > 0 && B > 0 && D > 0, "fx3d_chamfer_workspace_bytes: empty input");
    *bytes = workspace_layout(make_plan(N, M, B, D), N, M, B, D).total;
    return FX3D_OK;
}

fx3d_status fx3d_chamfer_sums(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                              int32_t D, double *sums_dev, int32_t *idx_x, int32_t *idx_y,
                              void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(sums_dev, "fx3d_chamfer_sums: null sums_dev");
    return chamfer_forward(x, N, y, M, B, D, sums_dev, nullptr, B, 1.f, 1.f, idx_x, idx_y, ws,
                           ws_bytes, as_stream(s), "fx3d_chamfer_sums");
}

fx3d_status fx3d_chamfer_finalize(const double *sums_dev, int32_t N, int32_t M, int64_t B_global,
                                  int32_t D, float w1, float w2, float *loss_dev,
                                  fx3d_stream_t s) {
    FX3D_REQUIRE(sums_dev && loss_dev, "fx3d_chamfer_finalize: null pointer");
    FX3D_REQUIRE(N > 0 && M > 0 && B_global > 0 && D > 0, "fx3d_chamfer_finalize: bad sizes");
    hipLaunchKernelGGL(chamfer_loss_kernel, dim3(1), dim3(64), 0, as_stream(s), sums_dev, N, M, D,
                       (long long)B_global, w1, w2, loss_dev);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_chamfer_finalize_many(const double *sums_dev, int32_t count, int32_t N, int32_t M, int64_t B_global,
                                       int32_t D, float w1, float w2, float *losses_dev, fx3d_stream_t s) {
    FX3D_REQUIRE(sums_dev && losses_dev, "fx3d_chamfer_finalize_many: null pointer");
    FX3D_REQUIRE(count > 0 && N > 0 && M > 0 && B_global > 0 && D > 0, "fx3d_chamfer_finalize_many: bad sizes");
    hipLaunchKernelGGL(chamfer_loss_many_kernel, dim3((count + 63) / 64), dim3(64), 0, as_stream(s), sums_dev, count, N, M,
                       D, (long long)B_global, w1, w2, losses_dev);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_chamfer_fwd(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                             int32_t D, float w1, float w2, float *loss_dev, float *loss_host,
                             int32_t *idx_x, int32_t *idx_y, void *ws, size_t ws_bytes,
                             fx3d_stream_t s) {
    FX3D_REQUIRE(loss_dev, "fx3d_chamfer_fwd: null loss_dev");
    fx3d_status rc = chamfer_forward(x, N, y, M, B, D, nullptr, loss_dev, B, w1, w2, idx_x, idx_y,
                                     ws, ws_bytes, as_stream(s), "fx3d_chamfer_fwd");
    if (rc) return rc;
    if (loss_host) {
        FX3D_HIP(hipMemcpyAsync(loss_host, loss_dev, sizeof(float), hipMemcpyDeviceToHost, as_stream(s)));
        FX3D_HIP(hipStreamSynchronize(as_stream(s)));
    }
    return FX3D_OK;
}

}  // extern "C"
