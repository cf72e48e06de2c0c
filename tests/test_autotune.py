"""The one per-shape kernel chooser (ops/autotune.py), driven without a device: a fake timer, a fake capture flag and
a temporary kernel-choice database stand in for the GPU."""
import json

import pytest

from deeplearning4j_amd.ops import autotune, side_stream, timing, tunedb


class Site:
    """A chooser call site with scripted launch statuses and kernel times; records what ``pick`` did with it."""

    def __init__(self, times, status=None):
        self.times, self.status = times, status or {}
        self.listed = self.defaulted = 0
        self.launched, self.timed, self.timer_args = [], [], []

    def candidates(self):
        self.listed += 1
        return list(self.times)

    def default(self):
        self.defaulted += 1
        return "dflt"

    def run(self, cand):
        self.launched.append(cand)
        return self.status.get(cand, 0)

    def pick(self, memo, key="k", **kw):
        return autotune.pick(memo, key, candidates=self.candidates, run=self.run, default=self.default, **kw)


@pytest.fixture
def env(tmp_path, monkeypatch):
    """Fresh tunedb state on an empty temporary database, no capture, and a timer that runs ``fn`` once and returns
    the scripted time of the candidate it launched."""
    monkeypatch.setattr(tunedb, "_db", None)
    monkeypatch.setattr(tunedb, "_recorded", {})
    monkeypatch.setattr(tunedb, "_path_used", None)
    monkeypatch.setattr(tunedb, "_cus", lambda: None)
    monkeypatch.delenv("DL4J_AMD_TUNE_DB_SKIP", raising=False)
    monkeypatch.delenv("DL4J_AMD_TUNE_REPS", raising=False)
    db = tmp_path / "db.json"
    monkeypatch.setenv("DL4J_AMD_TUNE_DB", str(db))
    monkeypatch.setattr(autotune, "capturing", lambda: False)
    monkeypatch.db = db
    return monkeypatch


def use_timer(monkeypatch, site):
    def gpu_time(fn, reps=3, warmup=1):
        n = len(site.launched)
        fn()
        cand = site.launched[n]
        site.timed.append(cand)
        site.timer_args.append((reps, warmup))
        return site.times[cand]
    monkeypatch.setattr(timing, "gpu_time", gpu_time)


def write_db(env, tables):
    env.db.write_text(json.dumps({"version": tunedb.VERSION, "arch": "gfx950", "cus": None, "tables": tables}))
    env.setattr(tunedb, "_db", None)


def recorded(table):
    return dict(tunedb._recorded.get(table, {}))


def test_memo_hit_calls_nothing(env):
    site = Site({"a": 1.0})
    use_timer(env, site)
    assert site.pick({"k": "a"}, table="t") == ("a", False)
    assert (site.listed, site.defaulted, site.launched, site.timed) == (0, 0, [], [])
    assert site.pick({"k": False}, table="t") == (False, False)          # a remembered False is a hit too
    assert (site.listed, site.defaulted, site.launched) == (0, 0, [])


def test_db_hit_is_memoised_and_never_timed(env):
    key = ("fwd", (1, 2), True)
    write_db(env, {"t": {repr(key): ["halo", 1, 16]}})
    site = Site({"a": 1.0})
    use_timer(env, site)
    memo = {}
    assert site.pick(memo, key, table="t") == (("halo", 1, 16), True)
    assert memo == {key: ("halo", 1, 16)}
    assert (site.listed, site.defaulted, site.launched, site.timed) == (0, 0, [], [])
    assert recorded("t") == {}
    assert site.pick(memo, key, table="t") == (("halo", 1, 16), False)    # now a memo hit


@pytest.mark.parametrize("how", ["capture", "disabled"])
def test_capture_or_disabled_returns_default_unremembered(env, how):
    site = Site({"a": 1.0})
    use_timer(env, site)
    memo = {}
    if how == "capture":
        env.setattr(autotune, "capturing", lambda: True)
        r = site.pick(memo, table="t")
    else:
        r = site.pick(memo, table="t", enabled=False)
    assert r == ("dflt", False)
    assert memo == {}
    assert recorded("t") == {}
    assert (site.listed, site.launched, site.timed) == (0, [], [])


def test_fastest_wins_and_is_memoised_and_recorded(env):
    site = Site({"a": 3.0, "b": 1.0, "c": 2.0})
    use_timer(env, site)
    memo = {}
    assert site.pick(memo, ("k", 1), table="t") == ("b", False)
    assert memo == {("k", 1): "b"}
    assert recorded("t") == {repr(("k", 1)): "b"}
    assert site.timed == ["a", "b", "c"] and site.defaulted == 0


def test_first_of_equal_times_wins(env):
    site = Site({"a": 2.0, "b": 1.0, "c": 1.0})
    use_timer(env, site)
    assert site.pick({}, table="t") == ("b", False)
    site = Site({True: 1.0, False: 1.0})
    use_timer(env, site)
    assert site.pick({}, table="t", probe=False)[0] is True


def test_refused_candidate_is_never_timed(env):
    site = Site({"a": 1.0, "b": 2.0}, status={"a": -4})
    use_timer(env, site)
    assert site.pick({}, table="t") == ("b", False)
    assert site.timed == ["b"]
    assert site.launched == ["a", "b", "b"]          # the probes of a and b, the timed launch of b


def test_status_one_needs_ok_to_list_it(env):
    site = Site({"a": 1.0, "b": 2.0}, status={"a": 1})
    use_timer(env, site)
    assert site.pick({}, table="t") == ("b", False)
    assert site.timed == ["b"]
    site = Site({"a": 1.0, "b": 2.0}, status={"a": 1})
    use_timer(env, site)
    assert site.pick({}, table="t", ok=(0, 1)) == ("a", False)
    assert site.timed == ["a", "b"]


def test_all_refused_takes_the_fallback(env):
    site = Site({"a": 1.0, "b": 2.0}, status={"a": -1, "b": -4})
    use_timer(env, site)
    memo = {}
    assert site.pick(memo, table="t", fallback=-1) == (-1, False)
    assert memo == {"k": -1}
    assert recorded("t") == {repr("k"): -1}
    assert site.timed == []
    memo = {}
    assert site.pick(memo, table="t") == ("dflt", False)      # no fallback given: the default is the choice
    assert memo == {"k": "dflt"} and recorded("t") == {repr("k"): "dflt"}


def test_no_table_touches_neither_lookup_nor_record(env):
    def boom(*a):
        raise AssertionError("tunedb used without a table")
    env.setattr(tunedb, "lookup", boom)
    env.setattr(tunedb, "record", boom)
    site = Site({"a": 2.0, "b": 1.0})
    use_timer(env, site)
    memo = {}
    assert site.pick(memo) == ("b", False)
    assert memo == {"k": "b"}


def test_probe_off_times_without_a_probe_launch(env):
    site = Site({"a": 2.0, "b": 1.0}, status={"b": -4})
    use_timer(env, site)
    assert site.pick({}, table="t", probe=False) == ("b", False)
    assert site.launched == ["a", "b"] and site.timed == ["a", "b"]        # only the timer launched


def test_reps_and_warmup_reach_the_timer(env):
    site = Site({"a": 1.0})
    use_timer(env, site)
    site.pick({}, "k1", table="t")
    site.pick({}, "k2", table="t", reps=2, warmup=0)
    env.setenv("DL4J_AMD_TUNE_REPS", "9")
    site.pick({}, "k3", table="t", reps=2)
    site.pick({}, "k4", table="t", reps=3, scale_reps=False)
    env.setenv("DL4J_AMD_TUNE_REPS", "1")
    site.pick({}, "k5", table="t", reps=3)
    assert site.timer_args == [(3, 1), (2, 0), (9, 1), (3, 1), (3, 1)]


def test_inline_suspends_the_overlap_stream_and_restores_it(env):
    state = {"dev": None, "main": None, "refs": [], "pending": False}
    env.setattr(side_stream._tl, "st", state, raising=False)
    seen = []

    class Inline(Site):
        def run(self, cand):
            seen.append(side_stream.active())
            return super().run(cand)
    site = Inline({"a": 1.0})
    use_timer(env, site)
    site.pick({}, "k1", table="t")
    assert seen == [True, True] and side_stream.active()
    del seen[:]
    site.pick({}, "k2", table="t", inline=True)
    assert seen == [False, False]
    assert side_stream._tl.st is state

    class Raising(Site):
        def run(self, cand):
            assert not side_stream.active()
            raise RuntimeError("launch failed")
    with pytest.raises(RuntimeError, match="launch failed"):
        Raising({"a": 1.0}).pick({}, "k3", table="t", inline=True)
    assert side_stream._tl.st is state


def test_db_skip_retimes_the_table(env):
    write_db(env, {"t": {repr("k"): "a"}, "u": {repr("k"): "a"}})
    env.setenv("DL4J_AMD_TUNE_DB_SKIP", "t")
    site = Site({"a": 2.0, "b": 1.0})
    use_timer(env, site)
    assert site.pick({}, table="t") == ("b", False)
    assert site.timed == ["a", "b"] and recorded("t") == {repr("k"): "b"}
    assert site.pick({}, table="u") == ("a", True)              # the other table is still served from the file
