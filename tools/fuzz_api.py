#!/usr/bin/env python3
"""Random CALL SEQUENCES of the host API on the GPU box, every result against the CPU oracle: tools/fuzz.py varies
configurations and always drives the same loop, this varies the calls (tests/api_sequences.py: generator, model, driver, the
buffer rule).  Sequence k of a run is the scenario of seed S + k.  Stops at the first sequence that fails or raises and
prints the line that replays it; never retries.

    python tools/fuzz_api.py --sequences 200 --seed 1000 [--size small|large] [--contexts 1|2] [--threads] [--seconds 500]
    python tools/fuzz_api.py --seed 1017 --sequences 1 --only 0        # one sequence, every operation with got and want
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--size", choices=["small", "large"], default="small")
    ap.add_argument("--contexts", type=int, choices=[1, 2], default=1)
    ap.add_argument("--threads", action="store_true", help="with --contexts 2: one context per thread instead of one merged order")
    ap.add_argument("--only", type=int, default=-1, help="replay sequence K alone and print every operation with got and want")
    ap.add_argument("--seconds", type=float, default=0.0, help="start no further sequence once this much time has passed (0: no limit)")
    ap.add_argument("--fake", action="store_true", help="drive the oracle-backed fake context instead of the library (no GPU)")
    args = ap.parse_args()
    import api_sequences as S
    if args.fake:
        factory = S.FakeHotPath
    else:
        import oat_amd
        factory = oat_amd.HotPath

    t0, done, sets = time.perf_counter(), 0, 0
    for k in range(args.sequences):
        if args.only >= 0 and k != args.only:
            continue
        if args.seconds and time.perf_counter() - t0 > args.seconds:
            break
        seed = args.seed + k
        if args.size == "large":
            seed %= len(S.LARGE_SHAPES)
        try:
            if args.contexts == 2 and args.threads:
                stats = S.run_on_two_threads(seed, factory, log=print if args.only >= 0 else None)
            elif args.contexts == 2:
                stats = S.run_interleaved(seed, factory, log=print if args.only >= 0 else None)
            else:
                stats = [S.run_scenario(S.scenario(seed, args.size), factory, log=print if args.only >= 0 else None).stats]
        except Exception as e:                                  # noqa: BLE001  (reported, then the run ends)
            print(f"FAILED sequence {k} (seed {seed}) after {done} good ones: {type(e).__name__}: {e}")
            if "replay:" not in str(e):
                print(f"replay: python tools/fuzz_api.py --seed {seed} --sequences 1 --only 0 --size {args.size}"
                      + (" --contexts 2" if args.contexts == 2 else "") + (" --threads" if args.threads else ""))
            sys.exit(1)
        done += 1
        sets += sum(st["collected"] for st in stats)
    print(f"fuzz_api: {done} sequences ({args.size}, {args.contexts} context(s){', threads' if args.threads else ''}) from seed "
          f"{args.seed}, {sets} result sets checked against the oracle, 0 failures, {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
