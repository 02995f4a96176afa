"""The failure-injection walk engine of tests/failure_walks.py, without a GPU and without a library: a fake stands in for the
library and for the shim, a toy scenario of three steps makes five creations, and the fake is bent one way per test so that each
judgement of run_case -- C1, C2, C3, C4, the shim's violations, the unexpected status -- is seen to report what it is there for.
On the GPU the walks only ever pass; here they are made to find something."""
import hashlib
import json

import pytest

from failure_walks import ERR_HIP, OK, Unexpected, logged_main, run_case, walk

SITES = (("a.cpp:10 hipMalloc", "a.cpp:11 hipHostMalloc"), ("b.cpp:20 hipEventCreateWithFlags",), ("c.cpp:30 hipMalloc", "c.cpp:31 hipStreamCreate"))
T = sum(len(s) for s in SITES)


class Ctx:
    def __init__(self):
        self.objs, self.error = [], b""


class Fake:
    """L and Shim in one: counts creations from mrt_fi_arm on, refuses the armed one, tracks what is live until mrt_destroy"""

    def __init__(self, **bends):
        self.ctxs, self.leaked, self.armed, self.calls, self.site = [], 0, 0, 0, None
        self.steps_called = []              # the toy scenario's call log, over all cases
        self.refusal_status = ERR_HIP       # what a refused creation makes its step return
        self.message = "{name}(&p, n) failed: out of memory"
        self.unsound = False                # mrt_debug_check_context fails once something was refused
        self.repeat_status = OK             # what a creation returns after the refusal
        self.stray_status = OK              # what step 1 returns although nothing was refused
        self.leak = False                   # mrt_destroy keeps one object of a context in which something was refused
        self.salt = ""                      # added to the observable of a case in which something was refused
        self.violation, self.always = None, False       # what violations() says once something was refused, or always
        self.__dict__.update(bends)

    def create(self, c, site):
        if self.site and self.repeat_status != OK:
            c.error = b"again"
            return self.repeat_status
        self.calls += 1
        if self.calls == self.armed:
            self.site = site
            c.error = self.message.format(name=site.split(" ")[1]).encode()
            return self.refusal_status
        c.objs.append(site)
        return OK

    # ---- the library
    def mrt_last_error(self, c):
        return c.error

    def mrt_debug_check_context(self, c, why, n):
        if self.unsound and self.site:
            why.value = b"a list is broken"
            return 1
        return 0

    def mrt_destroy(self, c):
        self.ctxs.remove(c)
        if self.leak and self.site:
            self.leaked += 1

    # ---- the shim
    def mrt_fi_reset(self):
        self.armed, self.calls, self.site = 0, 0, None

    def mrt_fi_arm(self, n):
        self.armed, self.calls = n, 0

    def mrt_fi_disarm(self):
        self.armed = 0

    def mrt_fi_calls(self):
        return self.calls

    def live(self):
        return [sum(len(c.objs) for c in self.ctxs) + self.leaked, 0, 0, 0]

    def fired(self):
        return self.site

    def violations(self):
        return [self.violation] if self.violation and (self.site or self.always) else []


class Toy:
    """three steps; each creates what it still lacks, as the library's `if (!p) hipMalloc(&p)` lines do"""
    root, what_differs = 0, "the toy's objects differ"

    def __init__(self, fake, repeat="act"):
        self.f, self.repeat = fake, repeat

    def prepare(self):
        self.f.ctxs.append(Ctx())
        return [self.f.ctxs[-1]]

    def steps(self, ctxs):
        def step(k):
            def run():
                self.f.steps_called.append(k)
                if k == 1 and self.f.stray_status != OK:
                    return self.f.stray_status
                for site in SITES[k]:
                    if site not in ctxs[0].objs:
                        st = self.f.create(ctxs[0], site)
                        if st != OK:
                            return st
                return OK
            return run
        return [step(k) for k in range(len(SITES))]

    def observe(self, ctxs):
        return hashlib.sha1((repr(ctxs[0].objs) + (self.f.salt if self.f.site else "")).encode()).hexdigest()


def run_walk(tmp_path, fake, repeat="act"):
    """(exit code, records) of a whole walk in logged_main"""
    log = tmp_path / "walk.jsonl"
    code = logged_main(log, lambda emit: walk(fake, fake, Toy(fake, repeat), emit))
    return code, [json.loads(line) for line in open(log)]


def refused(fake, n, repeat="act"):
    """the record of the case that refuses creation n, after a clean case"""
    _, clean_obs = run_case(fake, fake, Toy(fake, repeat), 0, None)
    fake.steps_called.clear()
    return run_case(fake, fake, Toy(fake, repeat), n, clean_obs)[0]


def test_a_clean_walk_counts_T_and_every_case_reaches_its_refusal(tmp_path):
    code, recs = run_walk(tmp_path, Fake())
    assert code == 0
    assert recs[0]["mode"] == "clean" and recs[0]["calls"] == T == 5 and not recs[0]["reached"]
    assert [r["n"] for r in recs[1:]] == list(range(1, T + 1)) and all(r["reached"] for r in recs[1:])
    assert [r["site"] for r in recs[1:]] == [s for step in SITES for s in step]
    assert not any(r["findings"] for r in recs)


def test_the_record_has_the_fields_the_drivers_read(tmp_path):
    _, recs = run_walk(tmp_path, Fake())
    assert set(recs[0]) == {"n", "mode", "findings", "calls", "reached"} and recs[0]["n"] == 0
    assert all(set(r) == {"n", "findings", "calls", "site", "reached"} for r in recs[1:])
    assert recs[3] == {"n": 3, "findings": [], "calls": 3, "site": SITES[1][0], "reached": True}


def test_a_refusal_with_another_status_is_a_C1_finding():
    rec = refused(Fake(refusal_status=5), 3)
    assert len(rec["findings"]) == 1 and rec["findings"][0].startswith(f"C1: the refusal at {SITES[1][0]} came back as status 5, not MRT_ERR_HIP")


def test_a_message_that_does_not_name_the_call_is_a_C1_finding():
    rec = refused(Fake(message="failed: out of memory"), 4)
    assert len(rec["findings"]) == 1 and rec["findings"][0].startswith(f"C1: mrt_last_error does not name the refused call hipMalloc at {SITES[2][0]}")
    rec = refused(Fake(message="{name} failed"), 4)             # the name alone, not the call
    assert len(rec["findings"]) == 1 and rec["findings"][0].startswith("C1: mrt_last_error does not name")


def test_an_unsound_context_is_a_C3_finding_and_gets_no_further_step():
    fake = Fake(unsound=True)
    rec = refused(fake, 3)
    assert rec["findings"] == [f"C3: after the refusal at {SITES[1][0]}: ctxs[0]: a list is broken"]
    assert fake.steps_called == [0, 1] and rec["reached"]


def test_a_repeat_that_fails_is_a_C4_finding():
    rec = refused(Fake(repeat_status=5), 3)
    assert rec["findings"] == [f"C4: repeated after the refusal at {SITES[1][0]}: status 5 (again)"]


def test_a_differing_observable_is_a_C4_finding_in_the_scenarios_words():
    rec = refused(Fake(salt="x"), 2)
    assert rec["findings"] == [f"C4: the toy's objects differ from the run in which nothing was refused (after {SITES[0][1]})"]


def test_something_live_after_destroy_is_a_C2_finding():
    rec = refused(Fake(leak=True), 5)
    assert rec["findings"] == ["C2: live {device, pinned, streams, events} [1, 0, 0, 0] after mrt_destroy, [0, 0, 0, 0] before mrt_create"]


def test_a_violation_the_shim_saw_is_reported():
    rec = refused(Fake(violation="hipFree of a pointer that is not live"), 1)
    assert rec["findings"] == ["shim: hipFree of a pointer that is not live"]


def test_a_status_that_was_not_injected_stops_the_walk(tmp_path):
    fake = Fake(stray_status=7)
    with pytest.raises(Unexpected, match="status 7 that the shim did not inject"):
        run_case(fake, fake, Toy(fake), 0, None)
    code, recs = run_walk(tmp_path, Fake(stray_status=7))
    assert code == 3 and len(recs) == 1 and "status 7 that the shim did not inject" in recs[0]["stopped"]


def test_any_other_exception_stops_the_walk_with_its_traceback(tmp_path):
    def body(emit):
        emit({"n": 0, "findings": []})
        raise KeyError("gone")
    log = tmp_path / "log.jsonl"
    assert logged_main(log, body) == 3
    recs = [json.loads(line) for line in open(log)]
    assert recs[1]["stopped"] == "exception: KeyError('gone')" and "KeyError" in recs[1]["traceback"]


def test_findings_give_exit_1_and_none_gives_exit_0(tmp_path):
    (tmp_path / "a").mkdir()
    code, recs = run_walk(tmp_path / "a", Fake(leak=True))
    assert code == 1 and len(recs) == T + 1 and all(r["findings"] for r in recs[1:]) and not recs[0]["findings"]
    (tmp_path / "b").mkdir()
    assert run_walk(tmp_path / "b", Fake())[0] == 0
    # a clean case with findings ends the walk there
    (tmp_path / "c").mkdir()
    code, recs = run_walk(tmp_path / "c", Fake(violation="double release", always=True))
    assert code == 1 and len(recs) == 1 and recs[0]["mode"] == "clean"


@pytest.mark.parametrize("n, act, step", [(3, [0, 1, 0, 1, 2], [0, 1, 1, 2]), (4, [0, 1, 2, 0, 1, 2], [0, 1, 2, 2]), (1, [0, 0, 1, 2], [0, 0, 1, 2])])
def test_the_repeat_starts_at_the_first_step_or_at_the_refused_one(n, act, step):
    for repeat, calls in (("act", act), ("step", step)):
        fake = Fake()
        rec = refused(fake, n, repeat)
        assert fake.steps_called == calls, repeat
        assert not rec["findings"] and rec["calls"] == n
