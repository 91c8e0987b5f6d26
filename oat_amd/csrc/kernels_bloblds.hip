// kernels_bloblds.hip -- K4'/K5': connected components, contour sums and the selection of a mostly empty frame by ONE workgroup
// a stream, on a run list in LDS (the global kernels of kernels_blob.hip take the frames it declines).
#include "oatgpu_internal.h"
#include "blobedges_inline.h"    // the contour-edge rule, the Green terms, the area window and key (+ blobruns_inline.h: lsb64)

namespace oatgpu {

// ------------------------------------------------------------ K4'/K5': one workgroup, in LDS ----
// Masks are mostly empty: after morphology a frame holds a few blobs, i.e. a few hundred "dirty" rows with three to
// five runs each.  Then ONE workgroup per stream does what k_merge + k_green_select do, on a run list in LDS: every
// dependent step of the union-find is an LDS access (~40 ns) instead of an L2 atomic (~270 ns, tools/atomic_latency.hip),
// and the three launches with their drain/fill become one.  k_rowscan supplies, per row, whether it holds foreground and
// how many runs (rowinfo), and per word the run starts before it (wpre).  Runs of a row alternate background /
// foreground starting with background (column 0 is zeroed), so run k of a row is foreground iff k is odd.
//   nodes: 0 = OUTSIDE; 1..R = the runs of the dirty rows in raster order (so the smallest node of a component is its
//   first pixel, the reference's tie-break key -- as in the global kernels).
//   A background run is OUTSIDE if it is the first or the last of its row, or if the row above or below is not dirty
//   (an all-background row is outside as a whole: both its ends are); otherwise it joins the background runs it
//   overlaps in the row above (4-connected).  Foreground runs join the foreground runs of the row above they touch
//   (8-connected: overlap widened by one pixel).
// Falls back (lds_ok = 0: k_merge + k_green_select take the frame) when the frame has more than kLdsRows dirty rows,
// kLdsRuns runs or kLdsRoots foreground components.
constexpr int kLdsRows = 1024, kLdsRuns = 3072, kLdsRoots = 768;      // 58 KB of LDS
// Threads of the one workgroup.  Beside the per-pixel kernel a launch of this kernel lasts 81-96 us at 4K in a kernel
// trace, against 21-27 us alone.  What the difference is (r03, tools/lds_phase_probe.py with a -DOATGPU_LDS_TIMING build:
// the kernel stamps the 100 MHz wall clock between its phases, profiles/r03j_backhalf_slot_wait.txt): the workgroup
// itself RUNS 26.3 us beside the per-pixel kernel and 25.5 us alone, phase for phase the same -- the other 55 us of
// the trace's duration pass before its first instruction: 16 waves with 61 KB of LDS need four free wave slots and
// 288 registers on every SIMD of ONE compute unit, the per-pixel kernel holds 8 waves / all 512 registers per SIMD
// everywhere and refills every slot a retiring 4-wave workgroup frees, and stream priority does not make the
// dispatcher hold slots back: the workgroup gets in when the running per-pixel launch drains (half a launch = 53 us
// on average).  (Earlier in r03 the duration was read as execution time and blamed on memory latency; the in-kernel
// clock refutes that, and so did removing this kernel's loads.)  Smaller workgroups do get in earlier but run longer:
// 512 / 256 threads 106 / 111 us and 16-21 % off the one-1080p-stream frame rate; s_setprio 3: no change.  Keeping the
// per-pixel kernel's stream off 4 / 8 / 16 compute units with a CU mask (hipExtStreamCreateWithCUMask) brings this
// kernel to 72 / 72 / 38 us and costs the per-pixel kernel 10 % whatever the number (107 -> 118 us per two-frame 4K
// launch, 17.5 k -> 15.9 k fps): not adopted.  A camera-bound pipeline never sees the wait: no later frame's
// per-pixel kernel is running when a frame's back half starts.
constexpr int kLdsBlock = 1024;
constexpr int kLdsTrip = 8;      // words of the run-start image a thread has in flight per trip of phase B

#ifdef OATGPU_LDS_TIMING           // measurement builds only (make variant DEFS=-DOATGPU_LDS_TIMING, tools/lds_phase_probe.py)
constexpr unsigned kLdsTkRing = 4096u;
__device__ long long g_lds_tk[kLdsTkRing * 10u];
__device__ unsigned g_lds_tk_n;
extern "C" __attribute__((visibility("default"))) int oatgpu_debug_lds_timing(long long *out, int max_rows)
{
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_lds_tk_n), sizeof n) != hipSuccess) return -1;
    const unsigned rows = n < kLdsTkRing ? n : kLdsTkRing;
    const unsigned take = rows < (unsigned)max_rows ? rows : (unsigned)max_rows;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lds_tk), (size_t)take * 10u * sizeof(long long)) != hipSuccess) return -1;
    return (int)take;
}
#endif

__device__ __forceinline__ int lds_find(int *par, int i)
{
    int cur = i, p = par[cur];
    while (p != cur) {
        const int gp = par[p];
        if (gp != p) atomicMin(&par[cur], gp);
        cur = p;
        p = gp;
    }
    return cur;
}
__device__ __forceinline__ void lds_union(int *par, int a, int b)
{
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

// Early dispatch (r04).  Beside the per-pixel kernel this kernel's one big workgroup used to WAIT ~55 us for 16 free wave
// slots on one compute unit (above) -- after its row scan had finished, i.e. on the frame's critical path.  With
// wait_ticket != 0 the launch sits on a HIP stream of its own and is submitted together with the frame's other kernels,
// long before the row scan runs: the workgroup takes its slots whenever the device has them (at the latest when the
// running per-pixel launch drains, one launch before it is needed), parks -- one lane polls b.ready[s] between
// s_sleeps, the other waves sit in the barrier and issue nothing; 16 of the chip's 8 192 wave slots -- and starts the
// moment k_rowscan's last workgroup publishes the ticket.  Should the ticket not come within kWaitTicks (a tool that
// serialises kernels, e.g. a counter-collecting profiler, makes the row scan wait for THIS kernel) the frame is
// declined like one that is too busy: the global kernels take it.
constexpr long long kWaitTicks = 10000000ll;         // 100 ms of the 100 MHz wall clock
template <typename T> __device__ __forceinline__ T ld_pub(const T *p)
{
    return __hip_atomic_load(const_cast<T *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// blockIdx.z selects one of TWO frames (scratch set, result record, ticket): the two frames of a two-frame step park
// their workgroups with ONE launch (launch_blob_tail2) -- two launches on one stream would run one after the other.
// TAB: the area window of plane s comes from tab[s] (k_rowscan)
template <bool TAB = false>
__global__ __launch_bounds__(kLdsBlock) void k_blob_lds(Geom g, BlobBuffers b0, BlobBuffers b1, double min_area, double max_area,
                                                        ResultRec *results0, ResultRec *results1, int first_stream, int spec,
                                                        unsigned ticket0, unsigned ticket1, const BlobTab *__restrict__ tab)
{
    __shared__ int wait_failed;
    const bool second = blockIdx.z != 0;
    const BlobBuffers &b = second ? b1 : b0;
    ResultRec *const results = second ? results1 : results0;
    const unsigned wait_ticket = second ? ticket1 : ticket0;
    __shared__ unsigned short rows[kLdsRows + 1];        // dirty row r -> image row
    __shared__ unsigned rptr[kLdsRows + 2];              // dirty row r -> its first node
    __shared__ unsigned short rstart[kLdsRuns + 2];      // node -> start x
    __shared__ unsigned short rrow[kLdsRuns + 2];        // node -> dirty row
    __shared__ int par[kLdsRuns + 2];
    __shared__ unsigned short rootslot[kLdsRuns + 2];
    __shared__ int rootnode[kLdsRoots];
    __shared__ unsigned long long acc[kLdsRoots * 3];
    __shared__ unsigned scan_d[kLdsBlock / 64], scan_r[kLdsBlock / 64];
    __shared__ unsigned nroots_s;
    __shared__ unsigned short fglist[kLdsRuns / 2 + 2];  // the foreground nodes, in any order (phase E walks these)
    __shared__ unsigned long long red[kLdsBlock / 64];

    const int s = first_stream + blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (TAB) { min_area = tab[s].min_area; max_area = tab[s].max_area; }
    const size_t soff = (size_t)s * (g.Palloc >> 6);
    const u64 *fin = b.fin + soff;
    const u64 *trans = b.trans + soff;
    const unsigned short *wpre = b.wpre + (size_t)s * g.H * g.words;
    const int *rowinfo = b.rowinfo + (size_t)s * g.H;

#ifdef OATGPU_LDS_TIMING
    long long tk[16]; int tn = 0;
#define TK() tk[tn++] = wall_clock64()
#else
#define TK()
#endif
    if (wait_ticket) {
        if (t == 0) {
            int bad = 0;
            const long long t0 = wall_clock64();
            while (__hip_atomic_load(&b.ready[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != wait_ticket) {
                // (somebody serialises kernel dispatches and a workgroup of this context has already waited its 100 ms in vain:
                // the host learns of it only when it collects that frame -- the frames parked behind it must not pay again)
                if (__hip_atomic_load(b.nopark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { bad = kPathNoPark; break; }
                __builtin_amdgcn_s_sleep(16);
                if (wall_clock64() - t0 > kWaitTicks) {
                    bad = kPathTimeout;
                    __hip_atomic_store(b.nopark, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
            wait_failed = bad;
        }
        __syncthreads();
        if (wait_failed) {
            if (t == 0) {
                b.lds_ok[s] = 0u;
                if (spec) { ResultRec r{}; r.first_pixel = -1; r.valid = kNeedsGlobal; r.path = wait_failed; results[s] = r; }
            }
            return;
        }
        // No acquire fence here: it is an L2 invalidate per wave, 16 per workgroup, on an XCD whose L2 the per-pixel kernel is
        // streaming through (measured: 4K per-pixel launch 104 -> 108 us, 16 x 1080p 403 -> 491 us).  Instead every load
        // of the row scan's arrays below is an agent-scope load (ld_pub): it is served by the memory side, where the row
        // scan's write-through stores are, whatever this XCD's L2 or this unit's L1 hold of an earlier frame.
    }
    TK();
    // ---- A: dirty rows and their run counts, in order (each thread owns a stretch of consecutive rows) ----
    const int per = (g.H + kLdsBlock - 1) / kLdsBlock;
    const int y0 = t * per, y1 = min(y0 + per, g.H);
    unsigned d = 0, rn = 0;
    // (r03: the row counts stay in registers for the second pass below when a thread owns <= 4 rows -- frames up to 4096
    // rows: every dependent global round trip of this kernel costs 4-5 us beside the per-pixel kernel, section header)
    int ric[4] = {0, 0, 0, 0};
    if (per <= 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int y = y0 + q; if (y < y1) ric[q] = ld_pub(rowinfo + y); }
#pragma unroll
        for (int q = 0; q < 4; ++q) if (ric[q]) { d++; rn += (unsigned)ric[q]; }
    } else {
        for (int y = y0; y < y1; ++y) { const int ri = ld_pub(rowinfo + y); if (ri) { d++; rn += (unsigned)ri; } }
    }
    unsigned di = d, ri_ = rn;                          // inclusive scans over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned vd = __shfl_up(di, o), vr = __shfl_up(ri_, o);
        if (lane >= o) { di += vd; ri_ += vr; }
    }
    if (lane == 63) { scan_d[wave] = di; scan_r[wave] = ri_; }
    if (t == 0) nroots_s = 0;
    __syncthreads();
    unsigned dbase = di - d, rbase = ri_ - rn, D = 0, R = 0;
    for (int i = 0; i < kLdsBlock / 64; ++i) {
        if (i < wave) { dbase += scan_d[i]; rbase += scan_r[i]; }
        D += scan_d[i]; R += scan_r[i];
    }
    if (D > (unsigned)kLdsRows || R > (unsigned)kLdsRuns) {          // too busy a frame for this path
        if (t == 0) {
            b.lds_ok[s] = 0u;
            if (spec) { ResultRec r{}; r.first_pixel = -1; r.valid = kNeedsGlobal; results[s] = r; }
        }
        return;
    }
    if (D == 0) {                                                     // nothing in the frame
        if (t == 0) {
            ResultRec r{};
            r.first_pixel = -1;
            r.path = 1;
            results[s] = r;
            b.lds_ok[s] = 1u;
        }
        return;
    }
    if (per <= 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ri = ric[q];
            if (ri) { rows[dbase] = (unsigned short)(y0 + q); rptr[dbase] = 1u + rbase; dbase++; rbase += (unsigned)ri; }
        }
    } else {
        for (int y = y0; y < y1; ++y) {
            const int ri = ld_pub(rowinfo + y);
            if (ri) { rows[dbase] = (unsigned short)y; rptr[dbase] = 1u + rbase; dbase++; rbase += (unsigned)ri; }
        }
    }
    if (t == 0) { rptr[D] = 1u + R; par[0] = 0; }
    __syncthreads();

    TK();
    // ---- B: the run list ----  (kLdsTrip words per thread and trip: the loads of a trip are in flight together)
    {
        const unsigned total = D * (unsigned)g.words;
        for (unsigned i0 = t; i0 < total; i0 += (unsigned)kLdsTrip * kLdsBlock) {
            u64 T[kLdsTrip];
            unsigned rr[kLdsTrip], pre[kLdsTrip];
            size_t gi[kLdsTrip];
#pragma unroll
            for (int u = 0; u < kLdsTrip; ++u) {
                const unsigned i = i0 + (unsigned)u * kLdsBlock, ic = min(i, total - 1u);   // (no branch round the load)
                const unsigned r = ic / (unsigned)g.words, w = ic - r * (unsigned)g.words;
                rr[u] = r;
                gi[u] = (size_t)rows[r] * g.words + w;
                T[u] = ld_pub(trans + gi[u]);
                pre[u] = ld_pub(wpre + gi[u]);
                if (i >= total) T[u] = 0ull;
            }
#pragma unroll
            for (int u = 0; u < kLdsTrip; ++u) {
                u64 Tu = T[u];
                if (!Tu) continue;
                const unsigned r = rr[u], w = (unsigned)(gi[u] - (size_t)rows[r] * g.words);
                unsigned node = rptr[r] + pre[u];
                while (Tu) {
                    const int bit = lsb64(Tu);
                    Tu &= Tu - 1;
                    rstart[node] = (unsigned short)(w * 64u + (unsigned)bit);
                    rrow[node] = (unsigned short)r;
                    par[node] = (int)node;
                    // (every row holds f foreground and f + 1 background runs: rows before r hold (rptr[r] - 1 - r) / 2
                    // foreground runs -- the list index needs no counter)
                    const unsigned kk = node - rptr[r];
                    if (kk & 1u) fglist[((rptr[r] - 1u - r) >> 1) + (kk >> 1)] = (unsigned short)node;
                    node++;
                }
            }
        }
    }
    __syncthreads();

    TK();
    // ---- C: unions ----
    for (unsigned i = 1 + t; i <= R; i += kLdsBlock) {
        const unsigned r = rrow[i], k = i - rptr[r];
        const int y = rows[r];
        const int sx = rstart[i], ex = (i + 1 < rptr[r + 1]) ? (int)rstart[i + 1] - 1 : g.W - 1;
        const bool adj_up = r > 0 && rows[r - 1] == y - 1, adj_dn = r + 1 < D && rows[r + 1] == y + 1;
        if (!(k & 1u)) {
            if (k == 0 || i + 1 == rptr[r + 1] || !adj_up || !adj_dn) lds_union(par, (int)i, 0);
            if (adj_up) {
                const unsigned je = rptr[r];
                for (unsigned j = rptr[r - 1]; j < je; j += 2) {
                    const int sj = rstart[j];
                    if (sj > ex) break;
                    const int ej = (j + 1 < je) ? (int)rstart[j + 1] - 1 : g.W - 1;
                    if (ej >= sx) lds_union(par, (int)i, (int)j);
                }
            }
        } else if (adj_up) {
            const unsigned je = rptr[r];
            for (unsigned j = rptr[r - 1] + 1; j < je; j += 2) {
                const int sj = rstart[j];
                if (sj > ex + 1) break;
                const int ej = (j + 1 < je) ? (int)rstart[j + 1] - 1 : g.W - 1;
                if (ej >= sx - 1) lds_union(par, (int)i, (int)j);
            }
        }
    }
    __syncthreads();

    TK();
    // ---- D: flatten; foreground roots get an accumulator slot ----
    int myroot[(kLdsRuns + kLdsBlock) / kLdsBlock];
#pragma unroll
    for (int q = 0; q < (kLdsRuns + kLdsBlock) / kLdsBlock; ++q) {
        const unsigned i = 1 + t + q * kLdsBlock;
        myroot[q] = i <= R ? lds_find(par, (int)i) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (kLdsRuns + kLdsBlock) / kLdsBlock; ++q) {
        const unsigned i = 1 + t + q * kLdsBlock;
        if (i <= R) {
            par[i] = myroot[q];
            if (myroot[q] == (int)i && ((i - rptr[rrow[i]]) & 1u)) {
                const unsigned slot = atomicAdd(&nroots_s, 1u);
                if (slot < (unsigned)kLdsRoots) {
                    rootslot[i] = (unsigned short)slot;
                    rootnode[slot] = (int)i;
                    acc[slot * 3] = 0ull; acc[slot * 3 + 1] = 0ull; acc[slot * 3 + 2] = 0ull;
                }
            }
        }
    }
    __syncthreads();
    const unsigned NR = nroots_s;
    if (NR > (unsigned)kLdsRoots) {
        if (t == 0) {
            b.lds_ok[s] = 0u;
            if (spec) { ResultRec r{}; r.first_pixel = -1; r.valid = kNeedsGlobal; results[s] = r; }
        }
        return;
    }

    TK();
    // ---- E: Green sums over the edges facing OUTSIDE background: 4 to 16 threads per foreground run, each taking its
    // share of the bits of every word (the per-bit loop is serial, and the top and bottom rows of a blob
    // are all border) ----
    const unsigned NF = (R - D) >> 1;
    // threads per run: 16, 8 or 4 -- as many as let all runs go in one pass (the per-bit loop below is serial and
    // ~300 instructions long; a thread takes 64 / lpr bits of every word)
    const int lpr_log = NF * 16u <= (unsigned)kLdsBlock ? 4 : (NF * 8u <= (unsigned)kLdsBlock ? 3 : 2);
    const int lpr = 1 << lpr_log, nbits = 64 >> lpr_log, sub = t & (lpr - 1);
    const int sh = nbits * sub;
    const u64 qbits = ((nbits == 64 ? ~0ull : ((1ull << nbits) - 1ull))) << sh;
    const unsigned qmask = (1u << nbits) - 1u;
    for (unsigned i0 = (unsigned)(t >> lpr_log); i0 < NF; i0 += (unsigned)(kLdsBlock >> lpr_log)) {
        const unsigned i = fglist[i0];
        const unsigned r = rrow[i];
        const int y = rows[r];
        const int sx = rstart[i], ex = (int)rstart[i + 1] - 1;       // a foreground run is never the last of its row
        const bool adj_up = r > 0 && rows[r - 1] == y - 1, adj_dn = r + 1 < D && rows[r + 1] == y + 1;
        const bool out_l = par[i - 1] == 0, out_r = par[i + 1] == 0;
        // run of row rr (a dirty neighbour row) that holds pixel x, memoised: [lo, hi] = its extent, root = its root
        struct Memo { int lo, hi, root; unsigned at; };
        Memo mu{1, 0, 0, adj_up ? rptr[r - 1] : 0u}, md{1, 0, 0, adj_dn ? rptr[r + 1] : 0u};
        auto root_at = [&](Memo &m, unsigned rr, int x) -> int {
            if (x >= m.lo && x <= m.hi) return m.root;
            unsigned j = (x > m.hi) ? m.at : rptr[rr];                // runs are visited left to right
            const unsigned je = rptr[rr + 1];
            while (j + 1 < je && (int)rstart[j + 1] <= x) ++j;
            m.at = j; m.lo = rstart[j]; m.hi = (j + 1 < je) ? (int)rstart[j + 1] - 1 : g.W - 1; m.root = par[j];
            return m.root;
        };
        long long s00 = 0, s10 = 0, s01 = 0;
        const size_t rc = (size_t)y * g.words, ru = rc - g.words, rd = rc + g.words;
#ifdef OATGPU_LDS_TIMING
        if (i0 == (unsigned)(t >> lpr_log)) { TK(); }
#endif
        // state of a neighbour row over [x0 - 1, x0 + 64] from the run list: 1 all foreground, 0 all OUTSIDE background,
        // 2 all background of a hole, -1 mixed (or the word is at the frame's edge)
        auto row_state = [&](Memo &m, unsigned rr, bool adj, int x0) -> int {
            if (!adj) return 0;                                       // the row is not in the list: no foreground, all outside
            const int rt = root_at(m, rr, x0);
            if (m.lo > x0 - 1 || m.hi < x0 + 64) return -1;
            if ((m.at - rptr[rr]) & 1u) return 1;
            return rt == 0 ? 0 : 2;
        };
        for (int w = sx >> 6; w <= (ex >> 6); ++w) {
            // A word strictly inside the run is all ones, and so are its left and right neighbours: its only edges are
            // straight top / bottom edges where the row above / below is outside background over the whole word -- known
            // from the run list in LDS, no load (r04: a run of n words cost n dependent round trips of loads per thread;
            // the full-frame blob of Oat's default window: 59 us of the kernel's 112).
            if (sx < w * 64 && ex > w * 64 + 63) {
                const int su = row_state(mu, r - 1, adj_up, w * 64), sd = row_state(md, r + 1, adj_dn, w * 64);
                if (su >= 0 && sd >= 0) {
                    if (su == 0 || sd == 0) {
                        const long long n = nbits, yy = y;
                        const long long sumx = n * (w * 64 + sh) + n * (n - 1) / 2;      // x over this thread's bits
                        if (su == 0) { s00 += n * yy; s10 += yy * (2 * sumx - n); s01 += 2 * yy * yy * n; }
                        if (sd == 0) { s00 -= n * yy; s10 -= yy * (2 * sumx + n); s01 -= 2 * yy * yy * n; }
                    }
                    continue;
                }
            }
            const int lo = max(sx - w * 64, 0), hi = min(ex - w * 64, 63);
            const u64 runbits = (hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull)) & ~((1ull << lo) - 1ull) & qbits;
            // the threads of a run need the same nine words: thread 0 of them fetches the run's row, thread 1
            // the row above, thread 2 the row below, and they pass them round (a quarter of the requests).
            // (r03: rebuilding the nine words from the run list in LDS instead -- no global load in this phase -- was
            // parity-green and no faster: 18.4 against 16.3 us alone at 1080p, 84 against 82 us beside the per-pixel
            // kernel at 4K, gpurun_out/bh1 -> profiles/r03j_backhalf_slot_wait.txt.  The loads are not what this
            // kernel waits for: see kLdsBlock.)
            const int role = sub;
            const size_t rbase = role == 0 ? rc : (role == 1 ? ru : rd);
            const bool hp = w > 0, hn = w + 1 < g.words;
            u64 m0 = 0ull, mP = 0ull, mN = 0ull;
            if (role < 3) {
                m0 = ld_pub(fin + rbase + w);
                mP = hp ? ld_pub(fin + rbase + w - 1) : 0ull;
                mN = hn ? ld_pub(fin + rbase + w + 1) : 0ull;
            }
            const int quad = lane & ~(lpr - 1);
            const u64 cur = __shfl(m0, quad), curP = __shfl(mP, quad), curN = __shfl(mN, quad);
            const u64 U = __shfl(m0, quad + 1), upP = __shfl(mP, quad + 1), upN = __shfl(mN, quad + 1);
            const u64 Dn = __shfl(m0, quad + 2), dnP = __shfl(mP, quad + 2), dnN = __shfl(mN, quad + 2);
            if (!runbits) continue;                                  // nothing of the run in this thread's bits
            // this thread's 16 bits of the nine masks as 32-bit values: the per-bit loop below is what the kernel's
            // time goes into (one compute unit runs it), and on 64-bit masks it was twice as many instructions
            const Ring<u64> n64 = ring_of(cur, curP, curN, U, upP, upN, Dn, dnP, dnN);
            auto q16 = [&](u64 v) -> unsigned { return (unsigned)(v >> sh) & qmask; };
            const unsigned cq = q16(cur & runbits);
            const Ring<unsigned> n{q16(n64.L), q16(n64.R), q16(n64.U), q16(n64.D), q16(n64.UL), q16(n64.UR), q16(n64.DL), q16(n64.DR)};
            const unsigned Lq = n.L, Rq = n.R, Uq = n.U, Dq = n.D;
            unsigned cand = cq & ~(Lq & Rq & Uq & Dq);
            const int xbase = w * 64 + sh;
            // Straight horizontal edges in closed form (r04).  A border pixel whose row above holds no foreground at all (the
            // row is not in the run list: everything there is OUTSIDE) and whose left neighbour is set contributes the top edge
            // (x, y) -> (x - 1, y): d = y, and the sums over a mask of such pixels need their count and the sum of their x --
            // four popcounts -- instead of one trip of the serial loop below each; the bottom edge (x, y) -> (x + 1, y)
            // likewise.  The top and the bottom row of a large blob are ALL such pixels: with Oat's default all-pass window
            // (one full-frame contour, the reference's own benchmark case) a thread walked up to 256 of them, 168 us a
            // 1 MP frame (profiles/r04x_posidet_default_trace.md).  Same int64 terms, same sums.
            unsigned ptop = 0u, pbot = 0u;
            if (!adj_up) ptop = cq & ~Uq & ~n.UL & Lq;
            if (!adj_dn) pbot = cq & ~Dq & ~n.DR & Rq;
            if (ptop | pbot) {
                auto sum_x = [&](unsigned m) -> long long {         // sum of x over the set bits of m
                    const int sb = __popc(m & 0xAAAAu) + 2 * __popc(m & 0xCCCCu) + 4 * __popc(m & 0xF0F0u) + 8 * __popc(m & 0xFF00u);
                    return (long long)__popc(m) * xbase + sb;
                };
                const long long nt = __popc(ptop), nb = __popc(pbot), yy = y;
                s00 += (nt - nb) * yy;
                s10 += yy * (2 * sum_x(ptop) - nt) - yy * (2 * sum_x(pbot) + nb);
                s01 += 2 * yy * yy * (nt - nb);
                // a pixel goes through the loop only for the sides that are left
                cand &= (~Lq | ~Rq | (~Uq & ~ptop) | (~Dq & ~pbot));
            }
            while (cand) {
                const int bi = __ffs((int)cand) - 1;
                cand &= cand - 1u;
                const int x = xbase + bi;
                const unsigned bit = 1u << bi;
                int qx, qy;
                // (qx, qy) is a neighbour of (x, y): |d| <= x + y < 2^15 (frames up to 16383 x 16383 take this path), the products fit 32 bits
                if (!(Lq & bit) && out_l && edge_end<kSideLeft>(n, bit, x, y, qx, qy)) green1<int>(x, y, qx, qy, s00, s10, s01);
                if (!((Dq | pbot) & bit) && (!adj_dn || root_at(md, r + 1, x) == 0) && edge_end<kSideBottom>(n, bit, x, y, qx, qy))
                    green1<int>(x, y, qx, qy, s00, s10, s01);
                if (!(Rq & bit) && out_r && edge_end<kSideRight>(n, bit, x, y, qx, qy)) green1<int>(x, y, qx, qy, s00, s10, s01);
                if (!((Uq | ptop) & bit) && (!adj_up || root_at(mu, r - 1, x) == 0) && edge_end<kSideTop>(n, bit, x, y, qx, qy))
                    green1<int>(x, y, qx, qy, s00, s10, s01);
            }
        }
        if (s00 | s10 | s01) {
            const unsigned slot = rootslot[par[i]];
            atomicAdd(&acc[slot * 3], (unsigned long long)s00);
            atomicAdd(&acc[slot * 3 + 1], (unsigned long long)s10);
            atomicAdd(&acc[slot * 3 + 2], (unsigned long long)s01);
        }
    }
#ifdef OATGPU_LDS_TIMING
    TK();
#endif
    __syncthreads();

    TK();
    // ---- F: the largest area in the window; ties go to the later first pixel (area_key) ----
    unsigned long long best = 0ull;
    for (unsigned q = t; q < NR; q += kLdsBlock) {
        const int node = rootnode[q];
        const unsigned h = (unsigned)rows[rrow[node]] * (unsigned)g.Wp + (unsigned)rstart[node];
        const unsigned long long key = area_key((long long)acc[q * 3], h, min_area, max_area);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(best, o);
        best = v > best ? v : best;
    }
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (t == 0) {
        u64 key = 0ull;
        for (int i = 0; i < kLdsBlock / 64; ++i) key = red[i] > key ? red[i] : key;
        ResultRec r{};
        r.first_pixel = -1;
        r.path = 1;
        if (key) {
            const unsigned h = key_first(key);
            // the root's slot: find it again (few roots)
            for (unsigned q = 0; q < NR; ++q) {
                const int node = rootnode[q];
                if ((unsigned)rows[rrow[node]] * (unsigned)g.Wp + (unsigned)rstart[node] == h) {
                    r.a00 = (long long)acc[q * 3]; r.a10 = (long long)acc[q * 3 + 1]; r.a01 = (long long)acc[q * 3 + 2];
                    break;
                }
            }
            r.first_pixel = first_pixel_of<unsigned>(g, h);
            r.valid = 1;
        }
        results[s] = r;
        b.lds_ok[s] = 1u;
#ifdef OATGPU_LDS_TIMING
        TK();
        // (a ring in device memory, read by oatgpu_debug_lds_timing: a printf here takes 400 us and turns "beside the
        // per-pixel kernel" into "alone")
        const unsigned slot = atomicAdd(&g_lds_tk_n, 1u) & (kLdsTkRing - 1u);
        for (int q = 0; q < 9; ++q) g_lds_tk[slot * 10u + q] = tk[q];
        g_lds_tk[slot * 10u + 9] = (long long)D << 32 | R;
#endif
    }
}

void launch_blob_lds(const Geom &g, int ny, int nz, const BlobBuffers &b0, const BlobBuffers &b1, double min_area, double max_area, ResultRec *results0,
                     ResultRec *results1, int first_stream, int spec, unsigned ticket0, unsigned ticket1, const BlobTab *tab, hipStream_t st)
{
    hipLaunchKernelGGL(tab ? k_blob_lds<true> : k_blob_lds<false>, dim3(1, ny, nz), dim3(kLdsBlock), 0, st, g, b0, b1, min_area, max_area,
                       results0, results1, first_stream, spec, ticket0, ticket1, tab);
}

}  // namespace oatgpu
