// kernels_rowscan.hip -- K2 / K3: morphology and the row scan, the front of posidet's back half on BIT-PACKED masks:
// cv::erode / cv::dilate, MORPH_RECT k x k (HSVDetector.cpp:152-156).
// A mask row is a string of 64-bit words (1 bit/pixel, 1080p row = 30 words); morphology is shifts and AND/OR on words.  The row
// scan applies it on the fly and leaves, per scratch set, what the connected-component kernels read: the final mask, its horizontal
// RUNS (run-start bits, the start of the run entering every word), the union-find initialised at run heads (kernels_blob.hip:
// k_merge, k_green_select) and the per-row run counts of the single-workgroup kernel (kernels_bloblds.hip: k_blob_lds).
#include "oatgpu_internal.h"
#include "blobruns_inline.h"     // msb64, lsb64, valid_bits

namespace oatgpu {

// ------------------------------------------------------------- morphology ----
// One thread = one output word.  Window of output bit x is [x-a, x-a+k-1] in
// both directions (a = k/2, not reflected); outside the image reads 1 for
// erosion and 0 for dilation (morphologyDefaultBorderValue).  k <= 63.
__global__ __launch_bounds__(256) void k_morph(Geom g, const u64 *src_all, u64 *dst_all, int k, int is_erode,
                                               int first_stream)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= g.H * g.words) return;
    const int s = first_stream + blockIdx.y;
    const int y = t / g.words, w = t - y * g.words;
    const u64 *src = src_all + (size_t)s * (g.Palloc >> 6);
    u64 *dst = dst_all + (size_t)s * (g.Palloc >> 6);
    const int a = k / 2;
    const u64 ident = is_erode ? ~0ull : 0ull;
    const u64 vlast = valid_bits(g, g.words - 1);

    u64 ap = ident, ac = ident, an = ident;
    for (int j = 0; j < k; ++j) {
        const int yy = y - a + j;
        if (yy < 0 || yy >= g.H) continue;          // border rows are the identity
        const u64 *row = src + (size_t)yy * g.words;
        u64 pw = w > 0 ? row[w - 1] : ident;
        u64 cw = row[w];
        u64 nw = (w + 1 < g.words) ? row[w + 1] : ident;
        if (is_erode) {                              // padding bits beyond x = W-1 read as 1
            if (w == g.words - 1) cw |= ~vlast;
            if (w + 1 == g.words - 1) nw |= ~vlast;
            ap &= pw; ac &= cw; an &= nw;
        } else {
            ap |= pw; ac |= cw; an |= nw;
        }
    }
    u64 out = ident;
    for (int j = 0; j < k; ++j) {
        const int o = j - a;                         // out bit i takes in bit i+o
        u64 v;
        if (o == 0) v = ac;
        else if (o > 0) v = (ac >> o) | (an << (64 - o));
        else v = (ac << (-o)) | (ap >> (64 + o));
        out = is_erode ? (out & v) : (out | v);
    }
    dst[(size_t)y * g.words + w] = out & valid_bits(g, w);
}

void launch_morph(const Geom &g, const u64 *src, u64 *dst, int k, bool is_erode, int first_stream,
                  int n_streams, hipStream_t st)
{
    const int n = g.H * g.words;
    hipLaunchKernelGGL(k_morph, dim3((n + 255) / 256, n_streams), dim3(256), 0, st, g, src, dst, k,
                       is_erode ? 1 : 0, first_stream);
}

// dilation of word (y, w) straight from the pre-dilation mask (same window rule as k_morph)
__device__ __forceinline__ u64 dilate_word(const Geom &g, const u64 *src, int y, int w, int k)
{
    const int a = k / 2;
    u64 ap = 0, ac = 0, an = 0;
    for (int j = 0; j < k; ++j) {
        const int yy = y - a + j;
        if (yy < 0 || yy >= g.H) continue;
        const u64 *row = src + (size_t)yy * g.words;
        if (w > 0) ap |= row[w - 1];
        ac |= row[w];
        if (w + 1 < g.words) an |= row[w + 1];
    }
    u64 out = 0;
    for (int j = 0; j < k; ++j) {
        const int o = j - a;
        out |= (o == 0) ? ac : (o > 0) ? ((ac >> o) | (an << (64 - o))) : ((ac << (-o)) | (ap >> (64 + o)));
    }
    return out & valid_bits(g, w);
}

// erosion of word (y, w) straight from the raw mask (same window rule as k_morph)
__device__ __forceinline__ u64 erode_word(const Geom &g, const u64 *src, int y, int w, int k)
{
    const int a = k / 2;
    const u64 vlast = valid_bits(g, g.words - 1);
    u64 ap = ~0ull, ac = ~0ull, an = ~0ull;
    for (int j = 0; j < k; ++j) {
        const int yy = y - a + j;
        if (yy < 0 || yy >= g.H) continue;
        const u64 *row = src + (size_t)yy * g.words;
        u64 cw = row[w];
        u64 nw = (w + 1 < g.words) ? row[w + 1] : ~0ull;
        if (w == g.words - 1) cw |= ~vlast;          // padding bits beyond x = W-1 read as 1
        if (w + 1 == g.words - 1) nw |= ~vlast;
        if (w > 0) ap &= row[w - 1];
        ac &= cw;
        an &= nw;
    }
    u64 out = ~0ull;
    for (int j = 0; j < k; ++j) {
        const int o = j - a;
        out &= (o == 0) ? ac : (o > 0) ? ((ac >> o) | (an << (64 - o))) : ((ac << (-o)) | (ap >> (64 + o)));
    }
    return out & valid_bits(g, w);
}

// dilation of word (rr, w) out of a block-local stack of eroded rows in LDS: row j of the
// window is er[(rr + j) * words + ...] (rows outside the image were stored as zeros)
__device__ __forceinline__ u64 dilate_word_lds(const Geom &g, const u64 *er, int rr, int w, int k)
{
    const int a = k / 2;
    u64 ap = 0, ac = 0, an = 0;
    for (int j = 0; j < k; ++j) {
        const u64 *row = er + (size_t)(rr + j) * g.words;
        if (w > 0) ap |= row[w - 1];
        ac |= row[w];
        if (w + 1 < g.words) an |= row[w + 1];
    }
    u64 out = 0;
    for (int j = 0; j < k; ++j) {
        const int o = j - a;
        out |= (o == 0) ? ac : (o > 0) ? ((ac >> o) | (an << (64 - o))) : ((ac << (-o)) | (ap >> (64 + o)));
    }
    return out & valid_bits(g, w);
}

// ------------------------------------------------------------- row scan ------
// One wavefront per image row at a time, one lane per mask word (rows wider than 4096 px
// loop in chunks of 64 words).  Applies the erosion (ERODE: the workgroup first
// erodes the ROWS + dil_k - 1 rows its dilation windows touch into LDS) and the
// dilation (dil_k > 1) on the fly, writes the final mask (image frame zeroed,
// as cvStartFindContours does in OpenCV 3.1), the run-start bits T, the start
// x of the run entering every word, and initialises the union-find at run heads.
//
// Workgroup shape: four waves, a row each.  Other shapes were measured beside the one-wave per-pixel launch of the early
// order (r07, profiles/r07a_rowscan_shape_ab.txt, r07e_rowscan_shape_ab.txt, r07h_timeline.txt): ONE wave a workgroup taking
// 4 / 2 / 1 rows in turn -- no earlier start, a longer chain per wave: gpu_total 243-263 -> 368-432 us; 8 / 16 waves a
// workgroup -- the whole launch runs in 16-21 us once it is in, but waits 60 us and more for room on one compute unit
// (it gets in when the per-pixel launch drains): no gain either.  The in-kernel clocks (tools/rowscan_probe.py, -DOATGPU_RS_TIMING)
// say where the 55-60 us of this kernel beside the per-pixel kernel go: a workgroup RUNS 7 us (9 p90), the 540 workgroups of a 4K
// frame START over 35 us -- the dispatcher hands this queue ~15 workgroups a microsecond while the per-pixel launch streams
// 1 300 a microsecond through the other.
// Rows a workgroup (ROWS, a template parameter: the loop over rows is the same at any height, and nothing a row writes depends on
// it, so steps of either height follow each other on the same scratch sets): 8 / 16 instead of 4 -- fewer workgroups beside K1, a
// longer loop in each -- disturbs K1 less: 4K 19.0 k -> 19.3 k / 19.6 k fps and one 1080p stream 56.2 k -> 56.8 k / 58.9 k; but a
// frame's result comes 40 / 83 us later (gpu_total 242 -> 282 / 325 us) and one frame at a time takes 127 -> 131 / 141 us:
// profiles/r07y_rowscan_rows_per_workgroup_ab.txt.  Where somebody waits for the frame that is a loss, and Oat is a real-time
// tracker: kRsRows = 4 is the default and what every single-stage call, the plain order, repairs and the marker table take.
// Where nobody can -- a step launched with four and more frames ahead of it in the ring, whose results are collected first --
// the later result costs nothing and the shorter period shortens the ring's latency too: such a step of the early or the
// paired order takes kRsRowsDeep (plan_step, api_track.hip; profiles/rowscan_deep_rows.txt).
constexpr int kRsWaves = 4, kRsRows = 4;
static_assert(kRsRows == kRsRowsNarrow && kRsRowsDeep % kRsWaves == 0, "oatgpu_internal.h names the same heights");

#ifdef OATGPU_RS_TIMING             // measurement builds only (make variant DEFS=-DOATGPU_RS_TIMING, tools/rowscan_probe.py)
constexpr unsigned kRsTkRing = 1u << 16;
__device__ long long g_rs_tk[kRsTkRing * 5u];       // {first instruction, last instruction, row group, tag} of a row group (100 MHz wall clock)
__device__ unsigned g_rs_tk_n;
__device__ const unsigned long long *g_rs_k1_end;   // where the per-pixel launches stamp the end of their last workgroups
void oatgpu_debug_rs_set_k1_end(const unsigned long long *p)
{
    static const unsigned long long *cur = nullptr;
    if (p != cur) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rs_k1_end), &p, sizeof p); cur = p; }
}
extern "C" __attribute__((visibility("default"))) int oatgpu_debug_rs_timing(long long *out, int max_rows)
{
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_rs_tk_n), sizeof n) != hipSuccess) return -1;
    const unsigned rows = n < kRsTkRing ? n : kRsTkRing;
    const unsigned take = rows < (unsigned)max_rows ? rows : (unsigned)max_rows;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rs_tk), (size_t)take * 5u * sizeof(long long)) != hipSuccess) return -1;
    return (int)take;
}
#endif
// blockIdx.z selects one of TWO frames (source mask, scratch set): the two frames of a two-frame step are scanned by ONE
// launch (launch_blob_pair: a launch is ~4 us of host time, and small frames are bound by exactly that).
// TAB (the marker sets' one back half for all markers, launch_blob_table): the planes of the launch are M x n planes of one
// geometry, and plane s takes its erode / dilate sizes from tab[s] -- a table in device memory, the index uniform over the
// workgroup, so the values arrive by scalar loads.  Always the ERODE form: an erosion of size 1 is the identity (a plane
// without erosion shares the launch with ones that have it; the LDS is sized by the launch's largest dilation), and the
// mask after erode / dilate is always written to b.morph.
template <bool ERODE, bool TAB = false, int ROWS = kRsRows>
__global__ __launch_bounds__(64 * kRsWaves) void k_rowscan(Geom g, const u64 *src0, const u64 *src1, int ero_k, int dil_k, BlobBuffers b0,
                                                        BlobBuffers b1, int first_stream, int clear_lds_ok, unsigned tag,
                                                        const BlobTab *__restrict__ tab)
{
    static_assert(ERODE || !TAB, "the table form erodes through LDS (size 1: the identity)");
    extern __shared__ u64 er[];
    constexpr int WAVES = kRsWaves;
    const bool second = blockIdx.z != 0;
    const BlobBuffers &b = second ? b1 : b0;
    const u64 *src_all = second ? src1 : src0;
    const int grp = blockIdx.x;                  // row group of this workgroup
    {
#ifdef OATGPU_RS_TIMING
    const long long rs_t0 = wall_clock64();
    const long long rs_k1_end_seen = g_rs_k1_end ? (long long)__hip_atomic_load(g_rs_k1_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ll;
#endif
    constexpr int NT = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int s = first_stream + blockIdx.y;
    const u64 *src_img = src_all + (size_t)s * (g.Palloc >> 6);
    if (TAB) { ero_k = tab[s].ero; dil_k = tab[s].dil; }       // (ero >= 1; dil 0 or > 1: launch_blob_table's caller)
    const int dk = dil_k > 1 ? dil_k : 1;
    if (ERODE) {
        const int r0 = grp * ROWS - dk / 2;
        const int n = (ROWS + dk - 1) * g.words;
        // Masks are mostly empty: if no bit is set in any row the erosion windows of this workgroup touch, the
        // eroded rows are zero (an image row never erodes to more than it holds) -- one pass over the source
        // words instead of ero_k x 3 loads per eroded word (4K, 7 x 7: 960 loads instead of 12 600 per workgroup).
        const int ya = max(r0 - ero_k / 2, 0), yb = min(r0 + (ROWS + dk - 1) - ero_k / 2 + ero_k - 1, g.H);   // source rows [ya, yb)
        u64 seen = 0ull;
        for (int i = ya * g.words + (int)threadIdx.x; i < yb * g.words; i += NT) seen |= src_img[i];
        const bool any = WAVES == 1 ? __ballot(seen != 0ull) != 0ull : __syncthreads_or(seen != 0ull) != 0;
        if (any) {
            for (int i = threadIdx.x; i < n; i += NT) {
                const int rr = i / g.words, w = i - rr * g.words;
                const int yy = r0 + rr;
                er[i] = (yy < 0 || yy >= g.H) ? 0ull : erode_word(g, src_img, yy, w, ero_k);
            }
        } else {
            for (int i = threadIdx.x; i < n; i += NT) er[i] = 0ull;
        }
        __syncthreads();
    }
    int *parent = b.parent + (size_t)s * g.Palloc;
    long long *acc = b.acc + (size_t)s * g.Palloc * 3;
    const int lastx = g.W - 1;

#pragma unroll 1
    for (int rr = wave; rr < ROWS; rr += WAVES) {
    const int y = grp * ROWS + rr;
    if (y >= g.H) break;
    const size_t woff = (size_t)s * (g.Palloc >> 6) + (size_t)y * g.words;
    u64 *morph = b.morph + woff;
    u64 *fin = b.fin + woff;
    u64 *trans = b.trans + woff;
    int *carry = b.carry + (size_t)s * g.H * g.words + (size_t)y * g.words;

    if (y == 0 && lane == 0) { b.nroots[s] = 0u; if (clear_lds_ok) b.lds_ok[s] = 0u; }

    const bool frame_row = (y == 0) || (y == g.H - 1);
    int chunk_carry = 0;        // start x of the last run seen so far
    u64 chunk_prevbit = 0;      // pixel value just left of this chunk
    unsigned short *wpre = b.wpre + ((size_t)s * g.H + y) * g.words;
    unsigned runs_before = 0;   // run starts of this row in earlier chunks
    bool row_fg = false;
    u64 keepT = 0ull, keepF = 0ull;   // rows of <= 64 words (<= 4096 px): the lane's T and F stay in registers for the loop below

    for (int c0 = 0; c0 < g.words; c0 += 64) {
        const int w = c0 + lane;
        const bool active = w < g.words;
        u64 F = 0;
        if (active && ERODE) {
            F = dilate_word_lds(g, er, rr, w, dk);   // dk == 1: the eroded word itself
            morph[w] = F;                            // the reference's threshold_frame_ (parity tap)
        } else if (active && dil_k > 1) {
            F = dilate_word(g, src_img, y, w, dil_k);
            morph[w] = F;
        } else if (active) {
            F = src_img[(size_t)y * g.words + w];
        }
        if (frame_row) F = 0;
        if (active && !frame_row) {
            F &= valid_bits(g, w);
            if (w == 0) F &= ~1ull;
            if (w == (lastx >> 6)) F &= ~(1ull << (lastx & 63));
        }
        // pixel left of bit 0: previous lane's bit 63
        u64 up = __shfl_up(F, 1);
        u64 prevbit = (lane == 0) ? chunk_prevbit : (up >> 63);
        u64 T = F ^ ((F << 1) | prevbit);
        if (w == 0) T |= 1ull;                       // a run starts at x = 0 by definition
        T &= valid_bits(g, w);
        if (!active) T = 0;

        const u64 nz = __ballot(T != 0);
        const u64 lower = nz & ((1ull << lane) - 1ull);
        const int pl = lower ? msb64(lower) : 0;
        const u64 Tp = __shfl(T, pl);
        const int cin = lower ? ((c0 + pl) * 64 + msb64(Tp)) : chunk_carry;

        // run starts in the words before this one (k_blob_lds places a row's runs with it)
        const unsigned cntT = (unsigned)__popcll(T);
        unsigned incl = cntT;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (active) {
            fin[w] = F;
            trans[w] = T;
            carry[w] = cin;
            wpre[w] = (unsigned short)min(runs_before + incl - cntT, 65535u);
        }
        keepT = T; keepF = F;
        runs_before += __shfl(incl, 63);
        row_fg = row_fg || __ballot(F != 0ull) != 0ull;
        // carry state into the next chunk (all lanes agree)
        if (nz) {
            const int hl = msb64(nz);
            const u64 Th = __shfl(T, hl);
            chunk_carry = (c0 + hl) * 64 + msb64(Th);
        }
        chunk_prevbit = __shfl(F, 63) >> 63;
    }

    // Union-find initialisation at run heads.  Column 0 and column W-1 are background in every
    // row (zeroed frame) and vertically 4-connected, so the first and the last run of every row
    // belong to the OUTSIDE component: hang them under root 0 right away -- on ordinary frames
    // this removes the H-long merge chain of full-width background runs.  Foreground run heads
    // get their Green accumulators cleared here.
    if (lane == 0) b.rowinfo[(size_t)s * g.H + y] = row_fg ? (int)runs_before : 0;
    const int last_start = chunk_carry;          // start x of the row's last run
    for (int c0 = 0; c0 < g.words; c0 += 64) {
        const int w = c0 + lane;
        if (w >= g.words) continue;
        // (written by this very lane above; re-read only when the row has more than one chunk -- the stores are write-
        // through, the loads were a global round trip of their own)
        u64 tt = g.words <= 64 ? keepT : trans[w];
        const u64 F = g.words <= 64 ? keepF : fin[w];
        while (tt) {
            const int i = lsb64(tt);
            tt &= tt - 1;
            const int sx = w * 64 + i;
            const int head = y * g.Wp + sx;
            parent[head] = (sx == 0 || sx == last_start) ? 0 : head;
            if ((F >> i) & 1ull) { acc[(size_t)head * 3] = 0; acc[(size_t)head * 3 + 1] = 0; acc[(size_t)head * 3 + 2] = 0; }
        }
    }
    }
#ifdef OATGPU_RS_TIMING
    if (threadIdx.x == 0 && blockIdx.y == 0) {
        const unsigned slot = atomicAdd(&g_rs_tk_n, 1u) & (kRsTkRing - 1u);
        g_rs_tk[slot * 5u] = rs_t0; g_rs_tk[slot * 5u + 1] = wall_clock64(); g_rs_tk[slot * 5u + 2] = grp; g_rs_tk[slot * 5u + 3] = tag;
        g_rs_tk[slot * 5u + 4] = rs_k1_end_seen;
    }
#else
    (void)tag;
#endif
    }
}

size_t rowscan_lds_bytes(const Geom &g, int dil_k)
{
    return (size_t)(kRsRows + (dil_k > 1 ? dil_k : 1) - 1) * g.words * sizeof(u64);
}

// ... and of a row scan of `rows` rows a workgroup (the rule a step must meet to take kRsRowsDeep: plan_step)
size_t rowscan_lds_bytes_rows(const Geom &g, int dil_k, int rows)
{
    return (size_t)(rows + (dil_k > 1 ? dil_k : 1) - 1) * g.words * sizeof(u64);
}

// the launch at a height other than kRsRows
template <int ROWS>
static void launch_rowscan_tall(const Geom &g, const u64 *const *src, int ero_k, int dil_k, const BlobBuffers *b, int nf, int first_stream,
                                int n_streams, int clear, hipStream_t st, unsigned tag)
{
    const int k = nf > 1 ? 1 : 0;
    const dim3 grid((g.H + ROWS - 1) / ROWS, n_streams, nf), block(64 * kRsWaves);
    if (ero_k > 1)
        hipLaunchKernelGGL((k_rowscan<true, false, ROWS>), grid, block, rowscan_lds_bytes_rows(g, dil_k, ROWS), st, g, src[0], src[k], ero_k,
                           dil_k, b[0], b[k], first_stream, clear, tag, nullptr);
    else
        hipLaunchKernelGGL((k_rowscan<false, false, ROWS>), grid, block, 0, st, g, src[0], src[k], 0, dil_k, b[0], b[k], first_stream, clear,
                           tag, nullptr);
}

// src / b: nf (1 or 2) frames' source masks and scratch sets; rows: kRsRows, or kRsRowsDeep where the caller has checked
// rowscan_lds_bytes_rows() against kRowscanLdsMax
void launch_rowscan(const Geom &g, const u64 *const *src, int ero_k, int dil_k, const BlobBuffers *b, int nf, int first_stream,
                    int n_streams, int clear, hipStream_t st, unsigned tag, int rows)
{
    if (rows == kRsRowsDeep) return launch_rowscan_tall<kRsRowsDeep>(g, src, ero_k, dil_k, b, nf, first_stream, n_streams, clear, st, tag);
#ifdef OATGPU_MEASURE               // the other candidate height of the A/B (OATGPU_RS_DEEP_ROWS, api_context.hip)
    if (rows == kRsRowsDeepAlt) return launch_rowscan_tall<kRsRowsDeepAlt>(g, src, ero_k, dil_k, b, nf, first_stream, n_streams, clear, st, tag);
#endif
    const int k = nf > 1 ? 1 : 0;
    const dim3 grid((g.H + kRsRows - 1) / kRsRows, n_streams, nf), block(64 * kRsWaves);
    if (ero_k > 1)
        hipLaunchKernelGGL(k_rowscan<true>, grid, block, rowscan_lds_bytes(g, dil_k), st, g, src[0], src[k], ero_k, dil_k, b[0], b[k],
                           first_stream, clear, tag, nullptr);
    else
        hipLaunchKernelGGL(k_rowscan<false>, grid, block, 0, st, g, src[0], src[k], 0, dil_k, b[0], b[k], first_stream, clear, tag, nullptr);
}

// the table form (TAB, above): n_planes planes of each of nf (1 or 2) frames, plane s with tab[s]'s sizes; max_dil sizes the LDS
void launch_rowscan_table(const Geom &g, const u64 *const *src, const BlobTab *tab, int max_dil, const BlobBuffers *b, int nf,
                          int n_planes, hipStream_t st)
{
    const int k = nf > 1 ? 1 : 0;
    hipLaunchKernelGGL((k_rowscan<true, true>), dim3((g.H + kRsRows - 1) / kRsRows, n_planes, nf), dim3(64 * kRsWaves),
                       rowscan_lds_bytes(g, max_dil), st, g, src[0], src[k], 0, 0, b[0], b[k], 0, 0, 0u, tab);
}

// The frame's ticket comes from a kernel of its own behind the row scan: the stream's order and the row scan's
// end-of-kernel release make its output visible to agent-scope loads, one lane per stream publishes.  (The in-kernel
// form -- k_rowscan storing what k_blob_lds reads write-through and its last-arriving workgroup publishing the ticket --
// saved that launch and cost the per-pixel kernel 3-4 %: profiles/r04o_*, r04p_*.)
__global__ void k_publish_ticket(unsigned *ready, int first_stream, unsigned ticket)
{
    __hip_atomic_store(&ready[first_stream + threadIdx.x], ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
void launch_rowscan_signal(const Geom &g, const BlobBuffers &b, const u64 *src_bits, int ero_k, int dil_k, int first_stream,
                           int n_streams, unsigned ticket, hipStream_t st, int rows)
{
    launch_rowscan(g, &src_bits, ero_k, dil_k, &b, 1, first_stream, n_streams, 0, st, ticket, rows);
    for (int s0 = 0; s0 < n_streams; s0 += 1024)
        hipLaunchKernelGGL(k_publish_ticket, dim3(1), dim3(n_streams - s0 < 1024 ? n_streams - s0 : 1024), 0, st, b.ready,
                           first_stream + s0, ticket);
}

}  // namespace oatgpu
