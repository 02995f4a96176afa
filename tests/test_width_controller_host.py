"""The launch-width controller's bookkeeping (csrc/width_policy.h, WidthController) over synthetic frame calls: CPU only, through
mrt_debug_width_replay.  tests/test_width_policy.py pins what a closed window decides; this file pins WHEN windows open and close,
what they measure, whom the controller believes about the frames in flight, and what it remembers -- the rules frames.cpp's
schedule_frame applied inline before, as its comments state them.  Like the policy, nothing here has a counterpart in the
reference (one draw per State::redraw).

A replay is one batch call on a fresh controller, so a script that has to react to a decision runs its calls so far again."""
import pytest

from test_width_policy import C1, C2, C3, C5_EIGHTH, INTERACTIVE

SLOTS = 1000            # lane slots a synthetic frame adds to the cumulative counter (Script.frame's `add`)
N_SPHERES = 488


class Script:
    """Frame calls in the making.  Call i is frame i; the counters of frame i - 1 land at call i unless the call says otherwise."""

    def __init__(self, mrt, workload, hint=None, probe_slots=0):
        self.mrt, self.workload, self.hint, self.probe_slots = mrt, tuple(workload) + (N_SPHERES,), hint, probe_slots
        self.calls, self.cum, self.t = [], [], 0.0

    def frame(self, util=0.80, dt=0.01, running=1, land="previous", add=SLOTS, **more):
        i = len(self.calls)
        self.t += dt
        hits, slots = self.cum[-1] if self.cum else (0, 0)
        self.cum.append((hits + round(util * add), slots + add))             # the cumulative counters after frame i's kernel
        seqs = ([i - 1] if i else []) if land == "previous" else list(land)
        self.calls.append(dict(now=self.t, running=running, samples=[(s, *self.cum[s]) for s in seqs], **more))
        return self

    def frames(self, n, **how):
        for _ in range(n):
            self.frame(**how)
        return self

    def run(self):
        return self.mrt.width_replay(self.workload, self.calls, self.hint, self.probe_slots)

    def last(self):
        return self.run()[-1]


def setting(d):
    return (d["div"], d["mult"])


def drive(script, behaviour, stop, limit=400, **how):
    """Frames (one at least), each with the (lane utilisation, frames / s) `behaviour` gives for the setting in force (None
    before the first call), until stop(decision)."""
    d = script.last() if script.calls else None
    while True:
        assert len(script.calls) < limit, "the script does not end"
        util, rate = behaviour(setting(d) if d else None)
        d = script.frame(util=util, dt=1.0 / rate, **how).last()
        if stop(d):
            return d


def closes(decisions):
    return [i for i, d in enumerate(decisions) if d["window_closed"]]


# ---- 1. the third generation ---------------------------------------------------------------------------------------------------

def test_no_window_before_the_third_generation_of_frames_and_no_sample_from_before_it(mrt):
    """C2 starts at (1, 1), two frames in flight: frames 0-1 start on an empty chip, 2-3 inherit their convoys, frame 4 is the
    first that counts (valid_from = frame + 2 x frames in flight).  Frames 0 to 4 run at utilisation 0, the later ones at 0.80;
    the samples of frames 2 and 3 land LATE, while the window is open: taken as its base, frame 4's zeros would be in the result."""
    s = Script(mrt, C2)
    s.frames(5, util=0.0, land=())
    s.frame(land=[4]).frame().frame(land=[2, 3, 6])
    s.frames(3)
    out = s.run()
    assert [d["window_open"] for d in out[:5]] == [0, 0, 0, 0, 1]
    assert closes(out) == [10]
    assert out[10]["util"] == pytest.approx(0.80, abs=1e-12)             # frames 5 to 9 over base = frame 4, last = frame 9
    # ... and the same again after the change of setting the window brought: (4, 2), eight in flight, 16 frames on
    assert setting(out[10]) == (4, 2) and not out[10]["window_open"]
    s.frames(18)
    out = s.run()
    assert [d["window_open"] for d in out[11:]] == [0] * 15 + [1] * 3    # opens at frame 10 + 2 x 8


# ---- 2. the window's length ----------------------------------------------------------------------------------------------------

def test_a_window_closes_after_twice_the_frames_in_flight_plus_two(mrt):
    s = Script(mrt, C2).frames(12)
    assert closes(s.run()) == [4 + 2 * 2 + 2]                            # opened at frame 4, (1, 1): two in flight
    eighth = Script(mrt, C1)                                             # C1: (1, 1) -> (1, 2): max(2, 1) x 2 = four in flight
    drive(eighth, lambda at: (0.60, 100.0), lambda d: setting(d) == (1, 2))
    first = len(eighth.calls) - 1
    eighth.frames(24)
    assert closes(eighth.run())[1] == (first + 2 * 4) + 2 * 4 + 2


def test_a_window_lasts_twenty_milliseconds_at_least(mrt):
    dt = 1.0 / 1024                                                      # (sums of it are exact)
    s = Script(mrt, C2).frames(40, dt=dt)
    out = s.run()
    assert closes(out) == [4 + 21]                                       # 20 / 1024 s < 0.020 s <= 21 / 1024 s: frames in plenty before
    assert all(d["window_open"] for d in out[4:25])
    assert out[25]["rate"] == pytest.approx(1024.0)


def test_a_window_needs_two_samples_that_differ(mrt):
    s = Script(mrt, C2).frames(5, land=())
    s.frame(land=[4]).frames(10, land=())                                # one sample: base and last on the same frame
    assert closes(s.run()) == [] and s.last()["window_open"]
    s.frame(land=[9])
    assert closes(s.run()) == [16]
    flat = Script(mrt, C2).frames(4).frames(13, add=0)                   # no lane slots between the samples
    assert closes(flat.run()) == [] and flat.last()["window_open"]
    assert closes(flat.frame().frame().run()) == [18]


# ---- 3. the two rates ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, kept", [(3, True), (4, False)])
def test_enough_device_intervals_replace_the_hosts_rate(mrt, n, kept):
    """C2's trial of (4, 2) after 200 frames / s at (1, 1): kept from 206 frames / s.  The host counts 236; eight slots whose
    start-to-start times sum to n x 8000 / 190 ms say 190.  max(2, 8 / 2) = 4 intervals are believed, 3 are not."""
    s = Script(mrt, C2)
    drive(s, lambda at: (0.80, 200.0), lambda d: setting(d) == (4, 2))
    before = len(closes(s.run()))
    d = drive(s, lambda at: (0.93, 236.0), lambda d: d["window_closed"], intervals=(n, n * 8000.0 / 190.0))
    assert len(closes(s.run())) == before + 1 and s.run()[-2]["frames_in_flight"] == 8
    if kept:
        assert d["rate"] == pytest.approx(236.0) and setting(d) == (4, 2) and not d["settled"] and d["util"] == pytest.approx(0.93)
    else:
        assert d["rate"] == pytest.approx(190.0) and setting(d) == (1, 1) and d["settled"]


# ---- 4. the frames the caller keeps in flight ----------------------------------------------------------------------------------

def test_the_running_window(mrt):
    s = Script(mrt, C5_EIGHTH, hint=None)                                # (8, 2): sixteen in flight
    assert s.frame(running=0).last()["frames_running"] == 15             # a new setting: "the caller keeps them all in flight"
    assert s.frame(running=3).last()["frames_running"] == 15
    assert s.frame(running=0).last()["frames_running"] == 15             # one call that sees nothing lowers nothing
    assert s.frame(running=0).last()["frames_running"] == 15
    assert s.frame(running=0).last()["frames_running"] == 0              # three in a row: a caller that waits for every frame
    assert s.frame(running=2).last()["frames_running"] == 2
    # the most over the last (frames in flight) calls: C2 at (1, 1) looks two calls back
    t = Script(mrt, C2)
    seen = [t.frame(running=r).last()["frames_running"] for r in (1, 1, 0, 1, 0, 0, 1)]
    assert seen == [1, 1, 1, 1, 1, 0, 1]


def test_a_change_of_setting_starts_the_running_window_over(mrt):
    s = Script(mrt, C2)
    d = drive(s, lambda at: (0.80, 200.0), lambda d: setting(d) == (4, 2), running=1)
    assert d["frames_running"] == 1                                      # (the count belongs to the frame launched at (1, 1) ...)
    out = s.frames(9, running=1).run()[-9:]
    assert [d["frames_running"] for d in out] == [7] * 7 + [1, 1]        # ... eight calls later the assumption has been replaced


# ---- 5. the memo ---------------------------------------------------------------------------------------------------------------

def c2_pays(at):
    return {(1, 1): (0.80, 200.0), (4, 2): (0.93, 236.0), (8, 2): (0.99, 237.0)}[at or (1, 1)]


def settled_c2(mrt):
    s = Script(mrt, C2)
    d = drive(s, c2_pays, lambda d: d["settled"])
    assert setting(d) == (4, 2) and d["memo_entries"] == 1
    return s


def test_a_settled_workload_comes_back_settled(mrt):
    s = settled_c2(mrt)
    n = len(s.calls)
    out = s.frame(invalidate=True).frames(40).run()[n:]
    assert all(setting(d) == (4, 2) and d["settled"] and not d["window_open"] and not d["window_closed"] for d in out)
    assert out[-1]["memo_entries"] == 1


@pytest.mark.parametrize("field, value", [(0, 150 * 84), (3, 32), (4, 2000), (5, 1), (6, N_SPHERES + 1)],
                         ids=["n_tiles", "spp", "large", "counter", "n_spheres"])
def test_another_workload_starts_the_trials_again(mrt, field, value):
    s = settled_c2(mrt)
    other = s.workload[:field] + (value,) + s.workload[field + 1:]
    d = s.frame(invalidate=True, workload=other).last()
    assert setting(d) == (1, 1) and not d["settled"]
    assert s.frames(4).last()["window_open"]


def test_settling_a_workload_again_replaces_its_entry(mrt):
    """No call of the library settles a remembered workload a second time (it comes back settled), but the entry is found by the
    workload the closing window is given: C2 settles at (1, 1); a frame at 32 samples per pixel starts the trials, and with C2
    back in force -- no setter in between -- they settle C2 at (4, 2)."""
    s = Script(mrt, C2)
    d = drive(s, lambda at: (0.97, 200.0), lambda d: d["settled"])
    assert setting(d) == (1, 1) and d["memo_entries"] == 1
    d = s.frame(invalidate=True, workload=s.workload[:3] + (32,) + s.workload[4:]).last()
    assert not d["settled"]
    s.frame(workload=s.workload)
    d = drive(s, lambda at: {(1, 1): (0.80, 200.0), (4, 2): (0.99, 236.0)}[at], lambda d: d["settled"])
    assert setting(d) == (4, 2) and d["memo_entries"] == 1
    d = s.frame(invalidate=True).last()
    assert setting(d) == (4, 2) and d["settled"] and d["memo_entries"] == 1


# ---- 6. the hint ---------------------------------------------------------------------------------------------------------------

def test_a_hint_is_the_setting_and_releasing_it_measures_again(mrt):
    s = Script(mrt, C3, hint=(4, 1)).frames(30)
    assert all(setting(d) == (4, 1) and d["settled"] and not d["window_open"] and d["frames_in_flight"] == 4 for d in s.run())
    d = s.frame(hint=(0, 0)).last()
    assert setting(d) == (2, 2) and not d["settled"]                     # what is known up front of C3
    assert closes(s.frames(30).run()) == [30 + 2 * 4 + 2 * 4 + 2]
    assert s.run()[30]["memo_entries"] == 0                              # (a hint leaves nothing in the memo)


def test_a_hint_keeps_its_width_within_the_slots_that_run_side_by_side(mrt):
    out = Script(mrt, C5_EIGHTH, hint=(8, 2), probe_slots=4).frames(3, running=3).run()
    assert all(setting(d) == (8, 2) and d["settled"] and d["frames_in_flight"] == 4 for d in out)
    assert [d["launch_div"] for d in out] == [8, 4, 4]                   # (from the second call on the running window holds 3)


# ---- 7. the probe's cap --------------------------------------------------------------------------------------------------------

def test_fewer_slots_than_sixteen_start_the_workload_over_within_them(mrt):
    s = Script(mrt, C5_EIGHTH, probe_slots=8).frames(18, running=7)
    out = s.run()
    assert all(setting(d) == (8, 1) and d["frames_in_flight"] == 8 and not d["settled"] for d in out)
    assert out[0]["frames_running"] == 15 and out[1]["frames_running"] == 7     # asked at (8, 2); the running window starts over
    assert [d["window_open"] for d in out] == [0] * 16 + [1] * 2                # ... and so does the measurement: 2 x 8 frames
    assert Script(mrt, C5_EIGHTH).frame().last()["frames_in_flight"] == 16      # (a probe that finds all sixteen changes nothing)


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------

def test_a_trial_that_pays_is_kept_and_the_next_one_is_reverted_through_whole_windows(mrt):
    """test_width_policy.py's test_a_trial_that_pays_is_kept_and_the_next_one_starts, by frame calls: C2 (1, 1) -> (4, 2) kept
    -> a second window at 0.93 -> (8, 2), + 0.4 %: reverted -> settled at (4, 2)."""
    s = Script(mrt, C2)
    drive(s, c2_pays, lambda d: d["settled"], running=15)
    out = s.run()
    path = [setting(out[0])] + [setting(out[i]) for i in closes(out)]
    assert path == [(1, 1), (4, 2), (4, 2), (8, 2), (4, 2)]
    assert [out[i]["settled"] for i in closes(out)] == [0, 0, 0, 1]
    assert [out[i]["util"] for i in closes(out)] == pytest.approx([0.80, 0.93, 0.93, 0.99], abs=1e-9)
    assert [out[i]["rate"] for i in closes(out)] == pytest.approx([200.0, 236.0, 236.0, 237.0])
    # every window: opened 2 x (frames in flight) after the setting, closed 2 x (frames in flight) + 2 later
    at, expect = 0, []
    for fif in (2, 8, 8, 16):
        at += 2 * fif + 2 * fif + 2
        expect.append(at)
    assert closes(out) == expect
    for d in out:
        assert d["launch_div"] == max(1, min(d["div"], d["frames_running"] + 1))
        assert d["frames_in_flight"] == max(2, d["div"]) * d["mult"]
    assert s.frame().last()["memo_entries"] == 1


def test_interactive_goes_on_from_a_quarter(mrt):
    """(test_width_policy.py's test_the_narrowest_launch_is_an_eighth by frame calls: the one start setting with mult 1 above a half)"""
    s = Script(mrt, INTERACTIVE)
    d = drive(s, lambda at: {(4, 1): (0.78, 3000.0), (8, 2): (0.89, 4100.0)}[at or (4, 1)], lambda d: d["settled"], running=15)
    assert setting(d) == (8, 2) and d["frames_in_flight"] == 16
