"""Every entry of the C ABI as the first call of a fresh context, on a veteran context, and alternating with itself at other sizes.

The rest of the suite runs on ONE session-wide context, whose grow-only arena, buffer pool and per-shape caches carry state from
test to test.  The invariant stated here: an entry, given the same arguments, returns the same bits and the same status whether it
is the first call its context sees or follows any other calls.  tests/fresh_probes.py holds the calls (one or more probes per
entry, a "main" and an "alt" variant each); three families run over that table:

  1. first call      a fresh context per probe runs "main" as its first engine call: it must return (an arena estimate below
                     what the entry carves shows here as "arena exhausted"), and where the route depends on the room the context
                     has, the result also meets the float64 bound of the entry's own test.  The result is kept as F[name].
  2. veteran         one context per entry group runs every "alt" (larger arena, pool and caches filled under other keys, stale
                     values 2^10 times larger), then every "main" in a shuffled order, trims, and runs every "main" again in
                     another order: all equal to F bit for bit.
  3. alternation     per probe on one context: alt, main, alt, main -- both "main" equal F, both "alt" equal each other --, then
                     near where the entry takes a value that is no size (a decay, a seed, a power ...): "near" keeps every size
                     of "main" and changes that value, the key a cache by shape would leave out.  A second fresh context runs
                     near, main, near: "near" equals itself whether it comes first or after "main", and "main" equals F after it.

and "main" on the suite's shared context equals F as well.  No tolerance appears in families 2 and 3.

Measured on an MI355X (docs/EXPERIMENTS.md, "Fresh-context probes"): 9.3 s for the 156 tests of this module on its own with one
context per alternation test; the second context of the 38 probes that have a "near" came after that measurement.  The module
creates 186 contexts one after the other (70 + 8 + 70 + 38: one per probe in family 1, one per group in family 2, one or two
per probe in family 3), 21 ms each; no test takes more than 2 s, all but the first (which loads the library) under 0.5 s.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fresh_probes as fp  # noqa: E402

pytestmark = pytest.mark.gpu

class _Fresh:
    """a context of its own, closed on the way out (before the next one is made)"""

    def __enter__(self):
        import torch

        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from xeofs_amd import engine

        self.ctx = engine.Context(0)
        return self.ctx

    def __exit__(self, *exc):
        import torch

        torch.cuda.synchronize()
        self.ctx.close()
        return False


@pytest.fixture(scope="session")
def first_results():
    """name -> F[name], the result of "main" as the first call of a fresh context; computed once, by whichever test asks first"""
    F = {}

    def get(name):
        if name not in F:
            with _Fresh() as c:
                F[name] = fp.BY_NAME[name].run(c, "main")
        return F[name]

    return get


def _assert_same(got, want, what):
    assert fp.same_bits(got, want), f"{what}: {fp.first_difference(got, want)}"


# ---------------------------------------------------------------------------------------------------------------- family 1
@pytest.mark.parametrize("name", [p.name for p in fp.PROBES])
def test_first_call_on_a_fresh_context(first_results, name):
    out = first_results(name)          # (raises MemoryError "arena exhausted" where a reserve is below its carve list)
    assert len(out) > 0 and all(isinstance(a, np.ndarray) for a in out)
    fp.BY_NAME[name].verify(out)


# ---------------------------------------------------------------------------------------------------------------- family 2
@pytest.mark.parametrize("group", fp.GROUPS)
def test_veteran_context(first_results, group):
    probes = [p for p in fp.PROBES if p.group == group]
    want = {p.name: first_results(p.name) for p in probes}
    rng = np.random.default_rng(len(probes))
    with _Fresh() as c:
        for p in probes:
            p.run(c, "alt")
        for order in range(2):
            for i in rng.permutation(len(probes)):
                _assert_same(probes[i].run(c, "main"), want[probes[i].name], f"{probes[i].name}, veteran context, order {order}")
            c.trim()


# ---------------------------------------------------------------------------------------------------------------- family 3
@pytest.mark.parametrize("name", [p.name for p in fp.PROBES])
def test_alternation(first_results, name):
    p = fp.BY_NAME[name]
    want = first_results(name)
    with _Fresh() as c:
        a1 = p.run(c, "alt")
        _assert_same(p.run(c, "main"), want, f"{name}, main after alt")
        _assert_same(p.run(c, "alt"), a1, f"{name}, alt after main against alt as the first call")
        _assert_same(p.run(c, "main"), want, f"{name}, main after alt, main, alt")
        near_after_main = p.run(c, "near") if "near" in p.cfg else None
    if near_after_main is not None:
        # the same sizes with another decay / seed / power ...: the key a cache is most likely to leave out.  Whichever of the two
        # comes first on a context fills the caches; each must come out as it does as a first call.
        with _Fresh() as c:
            n1 = p.run(c, "near")
            _assert_same(near_after_main, n1, f"{name}, the sizes of main with other values, after main, against the same as a first call")
            _assert_same(p.run(c, "main"), want, f"{name}, main after the same sizes with other values")
            _assert_same(p.run(c, "near"), n1, f"{name}, the sizes of main with other values, again after main")


# ------------------------------------------------------------------------------------------------- the suite's own context
@pytest.mark.parametrize("group", fp.GROUPS)
def test_shared_session_context(ctx, first_results, group):
    for p in fp.PROBES:
        if p.group == group:
            _assert_same(p.run(ctx, "main"), first_results(p.name), f"{p.name}, the session's context")
