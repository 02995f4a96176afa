#!/usr/bin/env python3
"""Dev helper (GPU box): a long campaign of random call sequences on one context against the host model, bit for bit.
   python scripts/state_campaign.py [n_cases] [first_case] [seconds] [--list]
The sequences and the runner are tests/state_sequences.py's (case numbers 0 .. are the suite's own).  Prints one line per
failing case and a summary; --list prints the sequences without touching the GPU or the oracle.  A status that is no
comparison failure (a stalled wait, a HIP error) ends the campaign there instead of going on to the next case."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import state_sequences as SS

def main():
    args = [a for a in sys.argv[1:] if a != "--list"]
    n_cases = int(args[0]) if len(args) > 0 else 200
    first = int(args[1]) if len(args) > 1 else 1000
    budget = float(args[2]) if len(args) > 2 else 1e9          # seconds: stop cleanly after this long
    if "--list" in sys.argv:
        for case in range(first, first + n_cases):
            p, ops = SS.sequence(case)
            print(f"case {case}: {p['width']}x{p['height']}x{p['spp']} depth {p['depth']} max_w {p['max_w']} seed {p['seed']}, {len(ops)} ops")
            for i, op in enumerate(ops):
                print(f"  {i:3d} {op!r}")
        return
    import myraytracer_amd as M
    from oracle import pyoracle as O
    fails, stats, t0, done, stopped = 0, {}, time.time(), 0, None
    for case in range(first, first + n_cases):
        p, _ = SS.sequence(case)
        try:
            with SS.new_state(p) as st:
                st.set_wait_timeout(60.0)
                SS.run(case, st, SS.new_model(O, p), stats)
        except SS.SequenceMismatch as e:
            fails += 1
            print(f"FAIL {str(e).splitlines()[0]}", flush=True)
            print(f"     {str(e).splitlines()[-1]}", flush=True)
        except (SS.SequenceStopped, M.MrtError) as e:
            stopped = f"STOPPED at case {case}: {e}"
            print(stopped, flush=True)
            done += 1
            break
        done += 1
        if done % 100 == 0:
            print(f"... {done} cases, {fails} failures, {time.time() - t0:.0f} s", flush=True)
        if time.time() - t0 > budget:
            break
    print(f"state campaign: cases {first} .. {first + done - 1} ({done}), {stats.get('ops', 0)} ops, {stats.get('frames', 0)} frames, "
          f"{fails} failures{', stopped early' if stopped else ''}, {time.time() - t0:.0f} s, build {M._lib.load().mrt_build_id().decode()}")
    sys.exit(2 if stopped else 1 if fails else 0)

if __name__ == "__main__":
    main()
