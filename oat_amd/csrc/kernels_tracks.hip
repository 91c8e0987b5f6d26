// kernels_tracks.hip -- target tracks: identity across frames for the K ranked blobs of a camera (oatgpu_set_tracks).
// k_target_tracks assigns one frame's ranked detections (k_blob_rank's target set, or the triples of oatgpu_tracks_update) to
// the K persistent track slots of every camera, runs each slot's Kalman filter and chain tail (chain_step, posfilt_inline.h: ONE
// definition) and publishes a twelve-word record a slot.  The semantics are the header's (include/oatgpu.h), step by step.
//
// One wave a camera stream.  Lanes 0..K-1 hold slot `lane` (its filter in registers, as k_tracker_filters holds a stream's) AND
// detection `lane`; lane i * 8 + j forms the cost of pair (slot i, rank j) from both by shuffles.  A greedy round is one
// wave-wide minimum over the pairs still open: a non-negative fp64 orders as its bit pattern, so the key is the cost's 64 bits
// and a closed or inadmissible pair is all ones; among equal keys the LOWEST LANE wins, which is the smaller slot, then the
// smaller rank -- the tie-break is the lane numbering.  At most K rounds.  The births are a few scalar steps on ballots, the same
// in every lane.  All fp64, one rounding per operation (-ffp-contract=off).  64-bit stores only.
#include "oatgpu_internal.h"
#include "posfilt_inline.h"

namespace oatgpu {

static_assert(sizeof(TrackRec) == 96, "twelve 64-bit words");
static_assert(kMaxTargets == 8, "lane i * 8 + j is pair (slot i, rank j)");

__global__ __launch_bounds__(64) void k_target_tracks(TrackLaunch a, const TargetRec *recs, const TrackTriple *tri, TrackRec *out)
{
    const int s = blockIdx.x, lane = threadIdx.x, K = a.k;
    const MarkerFilterParams *__restrict__ p = a.params;
    const KalmanLaunch k = chain_kalman(p, a.state);
    const size_t mine = (size_t)s * K + (lane < K ? lane : 0);      // (lanes K.. never touch memory through it)
    KalmanState *ks = a.state + mine;
    TrackMeta *km = a.meta + mine;

    // 1, 2: the slot's filter as the frame before left it, whether it is live, and where it expects its object; and detection `lane`
    Filter f{};
    TrackMeta m{0, 0, 0};
    int live = 0, det = 0;
    double px = 0.0, py = 0.0, cx = 0.0, cy = 0.0;
    if (lane < K) {
        load_filter(f, ks);
        m.id = __hip_atomic_load(&km->id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        m.age = __hip_atomic_load(&km->age, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        m.missed = __hip_atomic_load(&km->missed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        live = f.found != 0;
        const double *rep = f.aliased ? f.statePre : f.reported;
        px = rep[0] + k.dt * rep[1];
        py = rep[2] + k.dt * rep[3];
        if (recs) {
            const TargetRec &t = recs[mine];
            ResultRec r{};
            r.a00 = t.a00; r.a10 = t.a10; r.a01 = t.a01; r.valid = t.valid;
            det = centroid_of(r, cx, cy) ? 1 : 0;                  // posidet's centroid: oatgpu_position.x / .y of oatgpu_targets
        } else {
            const TrackTriple &t = tri[mine];
            det = t.valid != 0;
            cx = det ? t.x : 0.0; cy = det ? t.y : 0.0;
        }
    }

    // 3: the cost of pair (i, j) in lane i * 8 + j; slots and ranks from K on are neither live nor valid
    const int i = lane >> 3, j = lane & 7;
    const double pxi = __shfl(px, i), pyi = __shfl(py, i), cxj = __shfl(cx, j), cyj = __shfl(cy, j);
    const int live_i = __shfl(live, i), det_j = __shfl(det, j);
    const double dx = cxj - pxi, dy = cyj - pyi;
    const double cost = dx * dx + dy * dy;
    const bool admissible = live_i && det_j && cost <= a.gate2;     // (a NaN cost compares false)
    constexpr u64 kClosed = ~0ull;
    u64 key = admissible ? (u64)__double_as_longlong(cost) : kClosed;

    // 4: greedy global nearest neighbour
    int rank = -1;                       // lanes 0..K-1: the rank slot `lane` takes this frame
    unsigned taken = 0;                  // ranks assigned so far (the same in every lane)
    for (int round = 0; round < K; ++round) {
        if (__ballot(key != kClosed) == 0) break;
        u64 best = key;
        for (int o = 32; o; o >>= 1) {
            const u64 other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        const int w = __ffsll((unsigned long long)__ballot(key == best)) - 1;
        const int wi = w >> 3, wj = w & 7;
        if (lane == wi) rank = wj;
        taken |= 1u << wj;
        if (i == wi || j == wj) key = kClosed;
    }

    // 5: births -- valid ranks still unassigned, in rank order, into the slots that were not live when the frame began, ascending
    const unsigned kmask = (1u << K) - 1u;
    unsigned todo = (unsigned)__ballot(det != 0) & kmask & ~taken;
    unsigned vacant = ~(unsigned)__ballot(live != 0) & kmask;
    long long next = __hip_atomic_load(a.next_id + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool born = false;
    while (todo && vacant) {
        const int bj = __ffs(todo) - 1, bi = __ffs(vacant) - 1;
        todo &= todo - 1u; vacant &= vacant - 1u;
        if (lane == bi) { rank = bj; born = true; m.id = next; m.age = 0; m.missed = 0; }
        ++next;
    }
    if (lane == 0) __hip_atomic_store(a.next_id + s, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // 6: one sample a slot, then homography -> region as the trackers' chain (no heading)
    const int from = rank < 0 ? 0 : rank;
    const double mx = __shfl(cx, from), my = __shfl(cy, from);
    if (lane >= K) return;
    const bool measured = rank >= 0;
    TrackRec *o = out + mine;
    chain_step(p, k, f, measured ? 1 : 0, 0, measured ? mx : 0.0, measured ? my : 0.0, 0.0, 0.0, &o->f);
    store_filter(f, ks);

    // 7: the slot's identity after the step
    if (f.found) {
        if (!born) { m.age += 1; m.missed = measured ? 0 : m.missed + 1; }
    } else {
        m.id = 0; m.age = 0; m.missed = 0; rank = -1;
    }
    __hip_atomic_store(&km->id, m.id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&km->age, m.age, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&km->missed, m.missed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u64 *w = reinterpret_cast<u64 *>(o);
    __hip_atomic_store(w + 9, (u64)m.id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 10, (u64)(unsigned)rank | (u64)(unsigned)m.age << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 11, (u64)(unsigned)m.missed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void launch_target_tracks(const TrackLaunch &a, const TargetRec *recs, const TrackTriple *tri, TrackRec *out, int n_streams,
                          hipStream_t st)
{
    hipLaunchKernelGGL(k_target_tracks, dim3(n_streams), dim3(64), 0, st, a, recs, tri, out);
}

}  // namespace oatgpu
