// kernels_blob.hip -- K4, K5 and the riders: the back half of posidet on BIT-PACKED masks, behind the row scan
// (kernels_rowscan.hip: morphology, runs), and the launchers of the whole back half.
//   cv::findContours(RETR_EXTERNAL, ...)          (DetectorFunc.cpp:41-43)
//   cv::moments(contour)                          (DetectorFunc.cpp:50)
//   the largest-area-in-window selection          (DetectorFunc.cpp:45-65)
//
// The reference follows borders sequentially.  Here the same numbers come from an order-free formulation (proved equal to the
// sequential one by the CPU tests, tests/test_oracle_contours_crosscheck.py):
//   * a mask row is a string of 64-bit words (1 bit/pixel, 1080p row = 30 words);
//   * connected components are found over horizontal RUNS, not pixels: the union-find node of a run is the raster index of its
//     first pixel, so the parent table is touched only at run heads.  Foreground runs merge 8-connected, background runs
//     4-connected, in the same pass;
//   * the root of every component is its smallest head = its first pixel in raster order, which is exactly the reference's
//     tie-break key; the background component of pixel 0 (root 0) is "outside" (the image frame is zeroed first, as OpenCV 3.1
//     does), anything else is a hole;
//   * each foreground pixel emits at most one directed polygon edge per side facing OUTSIDE background (blobedges_inline.h: the
//     rule, once, for these kernels and for kernels_bloblds.hip's k_blob_lds, which takes the mostly empty frames in one
//     workgroup); exact int64 Green sums per root.
#include "oatgpu_internal.h"
#include "blobedges_inline.h"    // the contour-edge rule, the border walk, the Green terms, the area window and key, the arrival
                                 // (+ blobruns_inline.h: run_head, run_head_w, uf_root, shared with the target-mask kernel)

namespace oatgpu {

// ------------------------------------------------------------ union-find -----
// All accesses to parent[] inside the merge / flatten kernels are agent-scope
// relaxed atomics: correct for any placement of workgroups on XCDs (per-XCD
// L2s and per-CU L1s are not coherent for plain accesses).
__device__ __forceinline__ int uf_ld(int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_min(int *p, int v)
{
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(int *parent, int i)
{
    int cur = i;
    int p = uf_ld(parent + cur);
    while (p != cur) {
        const int gp = uf_ld(parent + p);
        if (gp != p) uf_min(parent + cur, gp);       // path halving (monotone, safe under races)
        cur = p;
        p = gp;
    }
    return cur;
}

__device__ __forceinline__ void uf_union(int *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }   // a > b: hang a under b
        const int old = uf_min(parent + a, b);
        if (old == a) return;                           // a was still a root
        a = old;                                        // lost a race: keep merging old with b
    }
}

// One thread = one word of row y (y >= 1): unite runs of row y with the runs
// of row y-1 they touch.  Background: 4-connected.  Foreground: 8-connected.
__global__ __launch_bounds__(256) void k_merge(Geom g, BlobBuffers b, int first_stream)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (g.H - 1) * g.words) return;
    const int s = first_stream + blockIdx.y;
    if (b.lds_ok[s]) return;                       // k_blob_lds took this frame
    const int y = 1 + t / g.words, w = t % g.words;
    const size_t soff = (size_t)s * (g.Palloc >> 6);
    const u64 *fin = b.fin + soff;
    const u64 *trans = b.trans + soff;
    const int *carry = b.carry + (size_t)s * g.H * g.words;
    int *parent = b.parent + (size_t)s * g.Palloc;

    const size_t rc = (size_t)y * g.words, ru = (size_t)(y - 1) * g.words;
    const u64 cur = fin[rc + w], up = fin[ru + w];
    const u64 curP = w > 0 ? fin[rc + w - 1] : 0ull;
    const u64 upP = w > 0 ? fin[ru + w - 1] : 0ull;
    const u64 upN = (w + 1 < g.words) ? fin[ru + w + 1] : 0ull;
    const u64 valid = valid_bits(g, w);
    const u64 Tc = trans[rc + w], Tu = trans[ru + w];
    const int cc = carry[rc + w], cu = carry[ru + w];

    // --- background, vertical contacts; one union per contact run ---
    u64 cb = ~cur & ~up & valid;
    if (w > 0 && (cb & 1ull) && (((~curP & ~upP) >> 63) & 1ull))
        cb &= cb + 1ull;                     // run continues from the previous word: its thread did it
    while (cb) {
        const int i = lsb64(cb);
        uf_union(parent, run_head_w(g, Tc, cc, y, w, i), run_head_w(g, Tu, cu, y - 1, w, i));
        cb &= cb + (cb & (~cb + 1ull));      // clear the lowest run of ones
    }
    if (cur == 0ull) return;

    // --- foreground, vertical contacts ---
    u64 cv = cur & up;
    if (w > 0 && (cv & 1ull) && (((curP & upP) >> 63) & 1ull))
        cv &= cv + 1ull;
    while (cv) {
        const int i = lsb64(cv);
        uf_union(parent, run_head_w(g, Tc, cc, y, w, i), run_head_w(g, Tu, cu, y - 1, w, i));
        cv &= cv + (cv & (~cv + 1ull));
    }
    // --- foreground, diagonal contacts not implied by a vertical one ---
    u64 dl = cur & ((up << 1) | (upP >> 63)) & ~up;   // up pixel at x-1
    while (dl) {
        const int i = lsb64(dl);
        dl &= dl - 1;
        uf_union(parent, run_head_w(g, Tc, cc, y, w, i), run_head(g, trans, carry, y - 1, w * 64 + i - 1));
    }
    u64 dr = cur & ((up >> 1) | (upN << 63)) & ~up;   // up pixel at x+1
    while (dr) {
        const int i = lsb64(dr);
        dr &= dr - 1;
        uf_union(parent, run_head_w(g, Tc, cc, y, w, i), run_head(g, trans, carry, y - 1, w * 64 + i + 1));
    }
}

// K5: contour sums + selection in ONE kernel.
// Phase 1, one thread = one word of an interior row:
//   * every foreground run head that is a root announces itself in the stream's root list;
//   * Green sums over the directed edges of foreground pixels that face OUTSIDE background
//     (root 0; walk_border), accumulated per root with int64 atomics.
// Phase 2, the last workgroup of the stream to arrive (arrive_last; everything it reads that
// this kernel wrote -- root list, sums -- is written and read with agent-scope atomics): every
// root offers its area_key; the maximum becomes the stream's result record in host-mapped memory.
// (kGreenChunks threads a mask word, kGreenBlock a workgroup: oatgpu_internal.h.)  TAB: the area window of plane s comes from tab[s] (k_rowscan)
template <bool TAB = false>
__global__ __launch_bounds__(kGreenBlock) void k_green_select(Geom g, BlobBuffers b, double min_area, double max_area,
                                                      ResultRec *results, int first_stream, const BlobTab *__restrict__ tab)
{
    __shared__ int is_last;
    __shared__ unsigned long long red[kGreenBlock];
    const int tt = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = first_stream + blockIdx.y;
    if (b.lds_ok[s]) return;                       // k_blob_lds took this frame (uniform over the workgroup)
    if (TAB) { min_area = tab[s].min_area; max_area = tab[s].max_area; }
    const size_t soff = (size_t)s * (g.Palloc >> 6);
    const u64 *fin = b.fin + soff;
    const u64 *trans = b.trans + soff;
    const int *carry = b.carry + (size_t)s * g.H * g.words;
    const int *parent = b.parent + (size_t)s * g.Palloc;
    long long *acc = b.acc + (size_t)s * g.Palloc * 3;
    int *roots = b.roots + (size_t)s * (g.Palloc >> 1);

    const BorderChunk c = border_chunk(g, fin, tt);
    if (c.any()) {
        const u64 Tc = trans[(size_t)c.y * g.words + c.w];
        // ---- roots announce themselves ----
        u64 heads = Tc & c.cur & c.bits;
        while (heads) {
            const int i = lsb64(heads);
            heads &= heads - 1;
            const int h = c.y * g.Wp + c.w * 64 + i;
            if (parent[h] == h) {
                const unsigned idx = __hip_atomic_fetch_add(&b.nroots[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(roots + idx, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // ---- Green sums: running sums a thread, flushed into the root's accumulators when the root changes ----
        int label = -1;
        long long s00 = 0, s10 = 0, s01 = 0;
        auto flush = [&]() {
            if (label >= 0 && (s00 | s10 | s01)) {
                atomicAdd((unsigned long long *)&acc[(size_t)label * 3], (unsigned long long)s00);
                atomicAdd((unsigned long long *)&acc[(size_t)label * 3 + 1], (unsigned long long)s10);
                atomicAdd((unsigned long long *)&acc[(size_t)label * 3 + 2], (unsigned long long)s01);
            }
        };
        Ring<u64> n;
        const u64 cand = border_bits(g, fin, c, n);
        walk_border(g, fin, trans, carry, parent, c, n, cand, Tc,
                    [&](int root) { flush(); label = root; s00 = s10 = s01 = 0; return true; },
                    [&](int x, int y, int qx, int qy) { green1<long long>(x, y, qx, qy, s00, s10, s01); },
                    [](int, int) {});
        flush();
    }

    // ---- arrival; the last workgroup of this stream selects ----
    if (!arrive_last(&b.done[s], &is_last)) return;

    const unsigned nr = __hip_atomic_load(&b.nroots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long best = 0ull;
    for (unsigned i = threadIdx.x; i < nr; i += blockDim.x) {
        const int h = __hip_atomic_load(roots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long a00 = __hip_atomic_load(&acc[(size_t)h * 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long key = area_key(a00, (unsigned)h, min_area, max_area);
        best = key > best ? key : best;
    }
    red[threadIdx.x] = best;
    __syncthreads();
    for (int st = kGreenBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st && red[threadIdx.x + st] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const u64 key = red[0];
        ResultRec r{};
        r.first_pixel = -1;
        if (key) {
            const int h = (int)key_first(key);
            r.a00 = __hip_atomic_load(&acc[(size_t)h * 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.a10 = __hip_atomic_load(&acc[(size_t)h * 3 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.a01 = __hip_atomic_load(&acc[(size_t)h * 3 + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.first_pixel = first_pixel_of<int>(g, h);
            r.valid = 1;
        }
        results[s] = r;
        __hip_atomic_store(&b.done[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void launch_blob(const Geom &g, const BlobBuffers &b, const u64 *src_bits, int ero_k, int dil_k, double min_area,
                 double max_area, ResultRec *results, int first_stream, int n_streams, hipStream_t st, int mode)
{
    const bool lds_able = g.H > 2 && g.H <= 16383 && g.W <= 16383;
    if (mode == kBlobSpec && !lds_able) mode = kBlobFull;
    const int clear = mode == kBlobGlobal || !lds_able;          // nobody else resets lds_ok then
    launch_rowscan(g, &src_bits, ero_k, dil_k, &b, 1, first_stream, n_streams, clear, st);
    if (lds_able && mode != kBlobGlobal)
        launch_blob_lds(g, n_streams, 1, b, b, min_area, max_area, results, results, first_stream, mode == kBlobSpec ? 1 : 0, 0u, 0u, nullptr, st);
    if (mode == kBlobSpec) return;
    if (g.H > 1)
        hipLaunchKernelGGL(k_merge, dim3(((g.H - 1) * g.words + 255) / 256, n_streams), dim3(256), 0, st, g, b, first_stream);
    // (grid of at least one workgroup even for H <= 2: the last-arriver logic writes the result)
    const int nw = (g.H > 2 ? (g.H - 2) * g.words : 1) * kGreenChunks;
    hipLaunchKernelGGL(k_green_select<false>, dim3((nw + kGreenBlock - 1) / kGreenBlock, n_streams), dim3(kGreenBlock), 0, st, g, b,
                       min_area, max_area, results, first_stream, nullptr);
}

// The back halves of the TWO frames of a step as two launches instead of four (speculative mode: row scan + the LDS
// kernel; a declined frame comes back marked kNeedsGlobal): frame i reads src[i] and scratch set b[i], writes results[i].
void launch_blob_pair(const Geom &g, const BlobBuffers *b, const u64 *const *src, int ero_k, int dil_k, double min_area,
                      double max_area, ResultRec *const *results, int n_streams, hipStream_t st, int rows)
{
    launch_rowscan(g, src, ero_k, dil_k, b, 2, 0, n_streams, 0, st, 0u, rows);
    launch_blob_lds(g, n_streams, 2, b[0], b[1], min_area, max_area, results[0], results[1], 0, 1, 0u, 0u, nullptr, st);
}

// The early blob workgroups of the nf (1 or 2) frames of a step in ONE launch: frame i reads scratch set b[i], writes
// results[i] and waits for ticket[i].  Speculative mode only (a declined frame comes back marked kNeedsGlobal).
void launch_blob_tail2(const Geom &g, const BlobBuffers *b, double min_area, double max_area, ResultRec *const *results,
                       int n_streams, const unsigned *ticket, int nf, hipStream_t st)
{
    const int k = nf > 1 ? 1 : 0;
    launch_blob_lds(g, n_streams, nf, b[0], b[k], min_area, max_area, results[0], results[k], 0, 1, ticket[0], ticket[k], nullptr, st);
}

// The marker sets' back half: the n_planes (= M x n) planes of each of the nf (1 or 2) frames of a step in ONE row-scan launch
// and ONE k_blob_lds launch (grid y = plane, z = frame), every plane with the erode / dilate / area of its table entry; the
// global kernels are queued behind them (a launch each a frame) and stand down on every plane the LDS kernel took, as in
// kBlobFull.  The number of launches does not depend on M.  Frame i reads src[i] ([n_planes][Palloc/64]) and scratch set b[i]
// (made for n_planes planes), writes results[i][n_planes].  LDS-able geometries only (launch_blob), and
// rowscan_lds_bytes(g, max_dil) <= kRowscanLdsMax, max_dil the largest dilation in the table: the caller checks both.
void launch_blob_table(const Geom &g, const BlobBuffers *b, const u64 *const *src, const BlobTab *tab, int max_dil,
                       ResultRec *const *results, int n_planes, int nf, hipStream_t st)
{
    const int k = nf > 1 ? 1 : 0;
    launch_rowscan_table(g, src, tab, max_dil, b, nf, n_planes, st);
    launch_blob_lds(g, n_planes, nf, b[0], b[k], 0.0, 0.0, results[0], results[k], 0, 0, 0u, 0u, tab, st);
    const int nw = (g.H - 2) * g.words * kGreenChunks;
    for (int i = 0; i < nf; ++i) {
        hipLaunchKernelGGL(k_merge, dim3(((g.H - 1) * g.words + 255) / 256, n_planes), dim3(256), 0, st, g, b[i], 0);
        hipLaunchKernelGGL(k_green_select<true>, dim3((nw + kGreenBlock - 1) / kGreenBlock, n_planes), dim3(kGreenBlock), 0, st, g,
                           b[i], 0.0, 0.0, results[i], 0, tab);
    }
}

// ------------------------------------------------------------ multi-target: the K largest blobs, ranked ----
// k_blob_rank runs on the HIP stream of a kBlobGlobal back half, directly behind it, on the same scratch set: k_green_select
// has left the first pixel of every foreground root in roots[0 .. nroots) and the Green sums of every one of them in acc
// (both stay until the set's next row scan), and has handed out only the maximum.  One workgroup a stream.
//   Candidates and ranking: area_key (blobedges_inline.h), the selection's own window and key: rank 0 is bit for bit the step's record.
//   One pass over the root list: every lane keeps the KC largest keys it has met, sorted, in registers (insertion by a
//     compare-exchange chain with constant indices).  Then k rounds of a workgroup maximum (wave shuffle, one LDS word a wave):
//     the lane whose head won pops it.  Keys are distinct (the first pixel is), so exactly one lane pops a round.  The order of
//     the root list differs from run to run; the ranking does not depend on it.
//   Output: k records a stream and the candidate count (which may exceed k), by 64-bit stores -- the target set
//     may be host-mapped memory.
constexpr int kRankBlock = 256;
template <int KC>
__global__ __launch_bounds__(kRankBlock) void k_blob_rank(Geom g, BlobBuffers b, double min_area, double max_area, int k,
                                                          TargetRec *__restrict__ recs, long long *__restrict__ found, int first_stream)
{
    static_assert(KC >= 1 && KC <= kMaxTargets, "a lane keeps at most kMaxTargets keys");
    __shared__ u64 red[kRankBlock / 64];
    __shared__ u64 win[kMaxTargets];
    __shared__ unsigned cnt[kRankBlock / 64];
    const int s = first_stream + blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long *acc = b.acc + (size_t)s * g.Palloc * 3;
    const int *roots = b.roots + (size_t)s * (g.Palloc >> 1);
    const unsigned nr = b.nroots[s];

    u64 top[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) top[i] = 0ull;
    unsigned mine = 0;
    for (unsigned i = threadIdx.x; i < nr; i += kRankBlock) {
        const int h = roots[i];
        u64 v = area_key(acc[(size_t)h * 3], (unsigned)h, min_area, max_area);
        if (!v) continue;
        ++mine;
#pragma unroll
        for (int q = 0; q < KC; ++q) {                    // top[] stays sorted, v leaves as the smallest of the KC + 1
            const u64 t = top[q];
            const bool up = v > t;
            top[q] = up ? v : t;
            v = up ? t : v;
        }
    }
    // the candidate count
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0) cnt[wave] = mine;

    for (int j = 0; j < k; ++j) {
        u64 best = top[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 v = __shfl_xor(best, o);
            best = v > best ? v : best;
        }
        if (lane == 0) red[wave] = best;
        __syncthreads();
        u64 key = red[0];
#pragma unroll
        for (int w = 1; w < kRankBlock / 64; ++w) key = red[w] > key ? red[w] : key;
        if (key != 0ull && top[0] == key) {
#pragma unroll
            for (int q = 0; q + 1 < KC; ++q) top[q] = top[q + 1];
            top[KC - 1] = 0ull;
        }
        if (threadIdx.x == 0) win[j] = key;
        __syncthreads();                                   // red[] is free for the next round, win[j] is visible
    }
    if (k == 0) __syncthreads();                           // cnt[]

    if ((int)threadIdx.x < k) {
        const u64 key = win[threadIdx.x];
        long long a00 = 0, a10 = 0, a01 = 0;
        int first_pixel = -1, valid = 0;
        if (key) {
            const int h = (int)key_first(key);
            a00 = acc[(size_t)h * 3]; a10 = acc[(size_t)h * 3 + 1]; a01 = acc[(size_t)h * 3 + 2];
            first_pixel = first_pixel_of<int>(g, h);
            valid = 1;
        }
        static_assert(sizeof(TargetRec) == 32, "a target record is four 64-bit words");
        u64 *o = reinterpret_cast<u64 *>(recs + (size_t)s * k + threadIdx.x);
        auto put = [&](int i, u64 v) { __hip_atomic_store(o + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        put(0, (u64)a00);
        put(1, (u64)a10);
        put(2, (u64)a01);
        put(3, (u64)(unsigned)first_pixel | (u64)(unsigned)valid << 32);
    }
    if (threadIdx.x == 0) {
        unsigned total = 0;
        for (int w = 0; w < kRankBlock / 64; ++w) total += cnt[w];
        __hip_atomic_store(found + s, (long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void launch_blob_rank(const Geom &g, const BlobBuffers &b, double min_area, double max_area, int k, TargetRec *recs,
                      long long *found, int first_stream, int n_streams, hipStream_t st)
{
    const dim3 grid(1, n_streams), block(kRankBlock);
    if (k <= 1) hipLaunchKernelGGL(k_blob_rank<1>, grid, block, 0, st, g, b, min_area, max_area, k, recs, found, first_stream);
    else if (k <= 4) hipLaunchKernelGGL(k_blob_rank<4>, grid, block, 0, st, g, b, min_area, max_area, k, recs, found, first_stream);
    else hipLaunchKernelGGL(k_blob_rank<kMaxTargets>, grid, block, 0, st, g, b, min_area, max_area, k, recs, found, first_stream);
}

// ------------------------------------------------------------ target shapes: order-2 sums and extents of the K ranked blobs ----
// k_blob_shape runs on the HIP stream of a kBlobGlobal back half directly behind its k_blob_rank, on the same scratch set: one more
// pass over the border pixels, for the K ranked roots only, launched only while shapes are on (oatgpu_set_target_shapes).
// What it relies on, and why that still holds the frame's data: fin, trans and carry are written by k_rowscan alone (k_morph,
//   k_merge, k_green_select, k_blob_lds, k_blob_rank and k_target_tracks only read them); parent is written by k_rowscan (run heads)
//   and by k_merge's unions and path halving, k_green_select walks it with plain loads (uf_root) and nothing behind k_merge writes
//   it; every launcher of this file issues these kernels on ONE HIP stream in the order row scan, merge, selection, and the host
//   launches the ranking and this kernel on that very stream before the set's next row scan (targets_launch, api_targets.hip).  So
//   all four hold the frame's final data from the end of k_merge until the set's next row scan -- as roots / acc do for k_blob_rank.
//   k_target_mask (crops_inline.h, kernels_targetmask.hip) relies on exactly this too: the batched trackers launch it
//   on that very stream behind the ranking (tracker_tail), it reads fin, trans, carry and parent with plain loads and writes none.
// The edges are k_green_select's (walk_border, blobedges_inline.h): one directed edge (x0, y0) -> (x1, y1) per side of a foreground
//   pixel that faces OUTSIDE background (root 0); an edge facing a hole is not one.  With d = x0 y1 - x1 y0, per ranked root (green2):
//     a20 += d (x0 (x0 + x1) + x1 x1)     a11 += d (x0 ((y0 + y1) + y0) + x1 ((y0 + y1) + y1))     a02 += d (y0 (y0 + y1) + y1 y1)
//   (contourMoments, imgproc/moments.cpp; exact in int64), and the extents are the extremes over the pixels that have a side facing outside.
// Grid: k_green_select's -- kGreenChunks threads a mask word, blockIdx.y = stream.  A workgroup none of whose chunks holds a border
//   bit goes straight to the arrival.  Otherwise the K ranked roots (padded indices, from TargetRec.first_pixel) are loaded
//   once a workgroup, a lane a rank, and read back uniformly from LDS; a border pixel's root is resolved first and the pixel is skipped unless it is one of the K;
//   only then are its four sides tested.  Running sums a thread, flushed on a label change into the workgroup's LDS accumulators
//   (64-bit LDS adds; the extents as unsigned maxima: INT_MAX - min), then ONE round of global atomics a touched rank into
//   accum[s][k][kShapeAccWords].  The last workgroup of the stream to arrive (arrive_last: each wave drains
//   vmcnt before arriving, the accumulator is written and read with agent-scope atomics) writes the stream's k ShapeRec by 64-bit
//   stores (the shape set may be host-mapped memory) and re-zeroes the accumulator and the counter for the slot's
//   next launch.  Integer sums and maxima: the result does not depend on the order of arrival.
static_assert(sizeof(ShapeRec) == 48, "a shape record is six 64-bit words");
template <int KC>
__global__ __launch_bounds__(kGreenBlock) void k_blob_shape(Geom g, BlobBuffers b, int k, const TargetRec *__restrict__ recs,
                                                            u64 *__restrict__ accum, unsigned *__restrict__ arrived,
                                                            ShapeRec *__restrict__ out, int first_stream)
{
    static_assert(KC >= 1 && KC <= kMaxTargets, "at most kMaxTargets ranks");
    __shared__ int is_last;
    __shared__ u64 lsum[kMaxTargets * 3];
    __shared__ unsigned lext[kMaxTargets * 4];
    __shared__ int lroot[kMaxTargets];
    const int tt = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = first_stream + blockIdx.y;
    const size_t soff = (size_t)s * (g.Palloc >> 6);
    const u64 *fin = b.fin + soff;
    const u64 *trans = b.trans + soff;
    const int *carry = b.carry + (size_t)s * g.H * g.words;
    const int *parent = b.parent + (size_t)s * g.Palloc;
    const TargetRec *tr = recs + (size_t)s * k;
    u64 *gacc = accum + (size_t)s * k * kShapeAccWords;

    if (threadIdx.x < kMaxTargets * 3) lsum[threadIdx.x] = 0ull;
    if (threadIdx.x < kMaxTargets * 4) lext[threadIdx.x] = 0u;

    const BorderChunk c = border_chunk(g, fin, tt);
    Ring<u64> n{};
    const u64 cand = c.any() ? border_bits(g, fin, c, n) : 0ull;
    if (__syncthreads_or(cand != 0ull)) {            // (uniform; also the barrier behind the LDS clears)
        // the K ranked roots: lane j fetches rank j -- the target set may be host-mapped memory, and K loads of one lane, one behind
        // the other, were K round trips over the link (profiles/shapes_bench.txt) -- and the workgroup reads them back uniformly
        if (threadIdx.x < kMaxTargets) {
            int r = -1;
            if ((int)threadIdx.x < k && tr[threadIdx.x].valid) {
                const int fp = tr[threadIdx.x].first_pixel, yy = fp / g.W;
                r = yy * g.Wp + (fp - yy * g.W);
            }
            lroot[threadIdx.x] = r;
        }
        __syncthreads();
        int root[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) root[j] = lroot[j];
        if (cand != 0ull && root[0] >= 0) {
            const int y = c.y;
            int rank = -1;
            long long s20 = 0, s11 = 0, s02 = 0;
            int x_lo = 0x7fffffff, x_hi = 0, y_hit = 0;
            auto flush = [&]() {
                if (rank >= 0 && y_hit) {
                    if (s20) atomicAdd((unsigned long long *)&lsum[rank * 3], (unsigned long long)s20);
                    if (s11) atomicAdd((unsigned long long *)&lsum[rank * 3 + 1], (unsigned long long)s11);
                    if (s02) atomicAdd((unsigned long long *)&lsum[rank * 3 + 2], (unsigned long long)s02);
                    atomicMax(&lext[rank * 4], 0x7fffffffu - (unsigned)x_lo);
                    atomicMax(&lext[rank * 4 + 1], 0x7fffffffu - (unsigned)y);
                    atomicMax(&lext[rank * 4 + 2], (unsigned)x_hi);
                    atomicMax(&lext[rank * 4 + 3], (unsigned)y);
                }
            };
            walk_border(g, fin, trans, carry, parent, c, n, cand, trans[(size_t)y * g.words + c.w],
                        [&](int lab) {
                            flush();
                            rank = -1;
#pragma unroll
                            for (int j = 0; j < KC; ++j) if (lab == root[j]) rank = j;
                            s20 = s11 = s02 = 0; x_lo = 0x7fffffff; x_hi = 0; y_hit = 0;
                            return rank >= 0;
                        },
                        [&](int x, int y, int qx, int qy) { green2(x, y, qx, qy, s20, s11, s02); },
                        [&](int x, int) { y_hit = 1; x_lo = x < x_lo ? x : x_lo; x_hi = x > x_hi ? x : x_hi; });
            flush();
        }
        __syncthreads();
        // one round of global atomics a touched rank
        if ((int)threadIdx.x < k * 3) {
            const u64 v = lsum[threadIdx.x];
            const int j = threadIdx.x / 3, q = threadIdx.x - j * 3;
            if (v) __hip_atomic_fetch_add(gacc + j * kShapeAccWords + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (threadIdx.x >= 64 && (int)threadIdx.x - 64 < k * 4) {
            const int i = threadIdx.x - 64, j = i >> 2, q = i & 3;
            const unsigned v = lext[i];
            if (v) __hip_atomic_fetch_max(reinterpret_cast<unsigned *>(gacc + j * kShapeAccWords + 3) + q, v, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- arrival; the last workgroup of this stream writes the records ----
    if (!arrive_last(&arrived[s], &is_last)) return;

    if ((int)threadIdx.x < k) {
        const int j = threadIdx.x;
        u64 *a = gacc + j * kShapeAccWords;
        u64 v[kShapeAccWords];
#pragma unroll
        for (int q = 0; q < kShapeAccWords; ++q) {
            v[q] = __hip_atomic_load(a + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a + q, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool valid = v[4] != 0ull;      // (a ranked blob has a pixel facing outside, x_max >= 1; an empty rank matched no pixel)
        u64 *o = reinterpret_cast<u64 *>(out + (size_t)s * k + j);
        auto put = [&](int i, u64 x) { __hip_atomic_store(o + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        const u64 lim = 0x7fffffffull;
        put(0, valid ? v[0] : 0ull);
        put(1, valid ? v[1] : 0ull);
        put(2, valid ? v[2] : 0ull);
        put(3, valid ? (lim - (v[3] & 0xffffffffull)) | (lim - (v[3] >> 32)) << 32 : 0ull);      // x_min | y_min << 32
        put(4, valid ? v[4] : 0ull);                                                              // x_max | y_max << 32
        put(5, valid ? 1ull : 0ull);
    }
    if (threadIdx.x == 0) __hip_atomic_store(&arrived[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void launch_blob_shape(const Geom &g, const BlobBuffers &b, int k, const TargetRec *recs, u64 *accum, unsigned *arrived,
                       ShapeRec *out, int first_stream, int n_streams, hipStream_t st)
{
    const int nw = (g.H > 2 ? (g.H - 2) * g.words : 1) * kGreenChunks;
    const dim3 grid((nw + kGreenBlock - 1) / kGreenBlock, n_streams), block(kGreenBlock);
    if (k <= 1) hipLaunchKernelGGL(k_blob_shape<1>, grid, block, 0, st, g, b, k, recs, accum, arrived, out, first_stream);
    else if (k <= 4) hipLaunchKernelGGL(k_blob_shape<4>, grid, block, 0, st, g, b, k, recs, accum, arrived, out, first_stream);
    else hipLaunchKernelGGL(k_blob_shape<kMaxTargets>, grid, block, 0, st, g, b, k, recs, accum, arrived, out, first_stream);
}

}  // namespace oatgpu
