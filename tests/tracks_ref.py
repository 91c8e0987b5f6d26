"""Target tracks (oatgpu_set_tracks) restated for the tests (TEST INFRASTRUCTURE, no GPU imports): the seven steps
of include/oatgpu.h in plain Python doubles, one oracle_lib.Kalman per slot -- kept for the life of a configuration -- and
marker_filters_ref.chain for the filtered part of every record.  Written from the header's text, not from the kernel.

A camera: Camera(k, kalman, gate, homography, regions).step(dets) with dets = k triples (valid, x, y) in rank order -> k records
(marker_filters_ref.chain's dict plus id, rank, age, missed), slot order.  Camera.log holds, per frame, what the step did -- the
non-vacuity checks of tests/test_tracks_cpu.py read it.  wrong= plants one of the WRONG trackers."""
import math

import marker_filters_ref as R
import oracle_lib as O

WRONG = ["rank_is_identity", "ties_to_higher_slot", "slot_order_nearest", "gate_ignored", "no_velocity", "births_into_freed",
         "ids_reused"]


class _Tap:
    """An oracle_lib.Kalman that remembers its latest output: the prediction of the next frame starts from it, in pixels, before
    any homography."""

    def __init__(self, **kw):
        self.kal, self.out = O.Kalman(**kw), None

    def filter(self, valid, x, y):
        self.out = self.kal.filter(valid, x, y)
        return self.out


class Camera:
    def __init__(self, k, kalman, gate=math.inf, homography=None, regions=None, wrong=None):
        assert 1 <= k <= 8 and gate >= 0
        self.k, self.gate, self.homography, self.regions, self.wrong = k, float(gate), homography, regions, wrong
        self.dt = float(kalman.get("dt", 0.02))
        self.threshold = int(float(kalman.get("timeout", 0.0)) / self.dt)
        self.kal = [_Tap(**kalman) for _ in range(k)]
        self.id, self.age, self.missed = [0] * k, [0] * k, [0] * k
        self.next_id = 1
        self.log = []

    # ---- steps 1 - 3 ----
    def live(self, i):
        o = self.kal[i].out
        return o is not None and o["position_valid"]

    def predicted(self, i):
        o = self.kal[i].out
        if self.wrong == "no_velocity":
            return o["x"], o["y"]
        return o["x"] + self.dt * o["vx"], o["y"] + self.dt * o["vy"]

    def cost(self, i, det):
        px, py = self.predicted(i)
        dx, dy = det[1] - px, det[2] - py
        return dx * dx + dy * dy

    def admissible(self, c):
        return not math.isnan(c) and (self.wrong == "gate_ignored" or c <= self.gate * self.gate)

    # ---- step 4 ----
    def assign(self, dets, live):
        k = self.k
        taken = {}                                   # slot -> rank
        if self.wrong == "rank_is_identity":
            return {i: i for i in range(k) if live[i] and dets[i][0]}, []
        pairs = [(self.cost(i, dets[j]), i, j) for i in range(k) if live[i] for j in range(k) if dets[j][0]]
        open_pairs = [p for p in pairs if self.admissible(p[0])]
        ties = []
        if self.wrong == "slot_order_nearest":
            for i in range(k):
                mine = sorted((c, j) for c, pi, j in open_pairs if pi == i and j not in taken.values())
                if mine:
                    taken[i] = mine[0][1]
            return taken, ties
        while True:
            left = [p for p in open_pairs if p[1] not in taken and p[2] not in taken.values()]
            if not left:
                return taken, ties
            if self.wrong == "ties_to_higher_slot":
                c, i, j = min(left, key=lambda p: (p[0], -p[1], p[2]))
            else:
                c, i, j = min(left)                  # the smallest cost, then the smaller slot, then the smaller rank
            if sum(1 for p in left if p[0] == c) > 1:
                ties.append((c, [p[1:] for p in left if p[0] == c]))
            taken[i] = j

    # ---- one frame ----
    def step(self, dets):
        k = self.k
        dets = [(bool(v), float(x), float(y)) for v, x, y in dets]
        assert len(dets) == k
        live = [self.live(i) for i in range(k)]
        taken, ties = self.assign(dets, live)
        gated = [j for j in range(k) if dets[j][0] and j not in taken.values() and any(live)
                 and all(self.cost(i, dets[j]) > self.gate * self.gate for i in range(k) if live[i])]
        # 5: births
        vacant = [i for i in range(k) if not live[i]]
        if self.wrong == "births_into_freed":        # ... and the slots whose track runs out on this very frame
            vacant = sorted(vacant + [i for i in range(k) if live[i] and i not in taken and self.missed[i] + 1 >= self.threshold])
        born, dropped = {}, []
        for j in range(k):
            if not dets[j][0] or j in taken.values():
                continue
            if not vacant:
                dropped.append(j)
                continue
            i = vacant.pop(0)
            born[i] = j
            if self.wrong == "ids_reused":
                new = next(n for n in range(1, 10 ** 6) if n not in self.id)
            else:
                new = self.next_id
                self.next_id += 1
            self.id[i], self.age[i], self.missed[i] = new, 0, 0
        # 6, 7: one sample a slot, the chain behind it, the identity behind that
        out, expired = [], []
        for i in range(k):
            j = taken.get(i, born.get(i, -1))
            m = dict(position_valid=j >= 0, x=dets[j][1] if j >= 0 else 0.0, y=dets[j][2] if j >= 0 else 0.0,
                     heading_valid=False, hx=0.0, hy=0.0)
            rec = R.chain(m, kalman=self.kal[i], homography=self.homography, regions=self.regions)
            if self.live(i):
                if i not in born:
                    self.age[i] += 1
                    self.missed[i] = 0 if j >= 0 else self.missed[i] + 1
            else:
                if self.id[i]:
                    expired.append(self.id[i])
                self.id[i], self.age[i], self.missed[i], j = 0, 0, 0, -1
            out.append(dict(rec, id=self.id[i], rank=j, age=self.age[i], missed=self.missed[i]))
        self.log.append(dict(live=live, taken=dict(taken), born=dict(born), dropped=dropped, gated=gated, ties=ties, expired=expired))
        return out


def run(frames, k, kalman, gate=math.inf, homography=None, regions=None, wrong=None):
    """out[t][i] over frames[t] = k triples, one camera from its start."""
    cam = Camera(k, kalman, gate, homography, regions, wrong)
    return [cam.step(d) for d in frames], cam.log


FLAGS = ("position_valid", "velocity_valid", "heading_valid", "region_valid", "region", "id", "rank", "age", "missed")
DOUBLES = ("x", "y", "vx", "vy", "hx", "hy")


def same(a, b):
    """two records agree: flags, region and identity exactly, doubles by == (NaN with NaN)"""
    return all(a[f] == b[f] for f in FLAGS) and all((math.isnan(a[d]) and math.isnan(b[d])) or a[d] == b[d] for d in DOUBLES)


def differs(a, b):
    return any(not same(x, y) for xs, ys in zip(a, b) for x, y in zip(xs, ys))
