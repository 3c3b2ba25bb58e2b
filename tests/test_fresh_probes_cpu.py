"""The probe table of the fresh-context tests (tests/fresh_probes.py) against include/eofx.h, without a GPU: every declared
entry has a probe or a written reason, the two variants of every probe differ in size, the shapes chosen for a route plan that
route, the comparison sees every bit, and the null-mode field has the rank its assertions count on."""

import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fresh_probes as fp  # noqa: E402
import plans_shim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_entries():
    """the names of every `int eofx_*(` declaration of the public header (names only)"""
    with open(os.path.join(ROOT, "include", "eofx.h")) as f:
        return set(re.findall(r"^\s*int\s+(eofx_\w+)\s*\(", f.read(), re.M))


def test_every_declared_entry_has_a_probe_or_a_reason():
    declared = declared_entries()
    assert len(declared) > 100
    probed = {e for p in fp.PROBES for e in p.entries}
    assert not probed & set(fp.EXEMPT), sorted(probed & set(fp.EXEMPT))
    assert probed | set(fp.EXEMPT) == declared, (sorted(declared - probed - set(fp.EXEMPT)), sorted((probed | set(fp.EXEMPT)) - declared))
    assert all(isinstance(r, str) and len(r) > 20 for r in fp.EXEMPT.values())


def test_no_probe_is_spare():
    """removing any probe from the table uncovers an entry, or a route that only this probe takes"""
    for drop in fp.PROBES:
        rest = {e for p in fp.PROBES if p is not drop for e in p.entries}
        assert (set(drop.entries) - rest) or drop.name in ROUTE_PROBES, drop.name     # (ROUTE_PROBES must all be there: below)


# the probes that share their entries with others and exist for a route of their own
ROUTE_PROBES = {"preprocess_copy", "preprocess_in_place", "preprocess_masked", "preprocess_raw", "products_f32", "products_f16x3", "products_f64", "tmul_nt",
                "cholqr_narrow", "cholqr_blocked", "rinv_blocked", "panel_gram", "matmul_narrow", "matmul_nt", "rot_step_narrow", "rot_step_wide",
                "rsvd_wide", "rsvd_tall", "rsvd_l70", "rsvd_full_width", "fit_fused", "fit_fallback", "fit_masked", "cross_gram_route",
                "cross_plain_route", "null_rsvd", "null_fit", "spca_loop_l1", "spca_loop_l0", "spca_loop_lds", "norms", "from_dense_download",
                "hilbert", "hilbert_small", "rsvd_c64", "rsvd_hilbert_c64"}


def test_names_are_unique_and_variants_differ():
    names = [p.name for p in fp.PROBES]
    assert len(set(names)) == len(names)
    assert ROUTE_PROBES <= set(names)
    for p in fp.PROBES:
        assert set(p.cfg) - {"near"} == set(fp.VARIANTS), p.name
        main, alt = p.cfg["main"], p.cfg["alt"]
        assert set(main) == set(alt), p.name
        sizes = [key for key in main if not isinstance(main[key], str) and key not in ("seed", "fused", "in_place", "standardize")]
        assert sizes and p.shape("main") != p.shape("alt"), p.name
        same = [key for key in sizes if main[key] == alt[key]]
        assert not same, (p.name, same)        # EVERY size parameter differs, not just one
        if "near" in p.cfg:                    # ... and "near" is "main" with one or two values changed, no more
            near = p.cfg["near"]
            assert set(near) == set(main) and 1 <= sum(near[key] != main[key] for key in main) <= 2, p.name


def test_inputs_are_seeded_and_alt_is_scaled():
    a, b = fp.Gen("x", "main"), fp.Gen("x", "main")
    assert np.array_equal(a.field(5, 7), b.field(5, 7))
    assert not np.array_equal(fp.Gen("x", "main").normal(9), fp.Gen("y", "main").normal(9))
    assert fp.Gen("x", "alt").scale == 2.0 ** 10 and fp.Gen("x", "main").scale == 1.0


def test_the_comparison_is_on_the_bits():
    a = (np.array([0.0, np.nan, 1.0], np.float32), np.array([3, 4], np.int32), np.asarray(2.5), np.array([1 + 2j], np.complex64))
    assert fp.same_bits(a, tuple(x.copy() for x in a)) and fp.first_difference(a, a) == "equal"      # NaN equals itself here
    for i, (j, value) in enumerate(((0, -0.0), (1, 5), ((), np.nextafter(2.5, 3.0)), (0, 1 - 2j))):
        b = [x.copy() for x in a]
        b[i][j] = value
        assert not fp.same_bits(a, tuple(b)) and fp.first_difference(a, tuple(b)).startswith(f"output {i} "), i
    assert not fp.same_bits(a, a[:3]) and not fp.same_bits(a[:1], (a[0].astype(np.float64),))
    assert not fp.same_bits(a[:1], (a[0].reshape(3, 1),))
    out = fp.host([dict(b=np.float32(1.5), a=3), (True, 2.0), None])
    assert [x.dtype.kind for x in out] == ["i", "f", "i", "f"] and [x.item() for x in out] == [3, 1.5, 1, 2.0]


def test_the_table_imports_without_torch():
    import subprocess

    code = "import sys; sys.path.insert(0, %r); import fresh_probes; assert 'torch' not in sys.modules and 'xeofs_amd' not in sys.modules"
    run = subprocess.run([sys.executable, "-c", code % os.path.dirname(os.path.abspath(__file__))], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]


def test_the_named_shapes_plan_the_routes_they_are_for():
    lib = plans_shim.lib()
    up = lambda x, m: (x + m - 1) // m * m          # noqa: E731
    kps = plans_shim.I64()
    for name in ("products_f32", "products_f16x3", "products_f64"):       # more than one K split in both directions
        for variant in fp.VARIANTS:
            c = fp.BY_NAME[name].params(variant)
            t = [lib.pl_atb_plan(up(p, 512), n, c.L, 0, plans_shim.ctypes.byref(kps)) for n, p in c.shapes]
            m = [lib.pl_atb_plan(up(n, 512), p, c.L, 0, plans_shim.ctypes.byref(kps)) for n, p in c.shapes]
            assert max(t) > 1 and max(m) > 1, (name, variant, t, m)
    for variant in fp.VARIANTS:
        c = fp.BY_NAME["tmul_nt"].params(variant)
        assert lib.pl_tmul_nt_ok(c.n, up(c.p, 512), 1, c.L)
        c = fp.BY_NAME["matmul_nt"].params(variant)
        assert lib.pl_matmul_nt_ok(c.rows, c.L, c.Lo)
        c = fp.BY_NAME["matmul_narrow"].params(variant)
        assert not lib.pl_matmul_nt_ok(c.rows, c.L, c.Lo)
    c = fp.BY_NAME["tmul_nt"].params("main")
    assert (c.n, c.p, c.L) == (700, 3000, 512)
    c = fp.BY_NAME["matmul_nt"].params("main")
    assert (c.rows, c.L, c.Lo) == (1024, 512, 260)
    for name, blocked in (("cholqr_narrow", False), ("cholqr_blocked", True), ("rinv_blocked", True)):
        for variant in fp.VARIANTS:
            assert (fp.BY_NAME[name].params(variant).l > 64) == blocked
    assert fp.BY_NAME["cholqr_blocked"].params("main").l == 70 and fp.BY_NAME["rsvd_l70"].params("main").k + 10 == 70
    for name in ("fit_fused", "fit_masked"):
        assert all(fp.BY_NAME[name].params(v).k + 10 <= 63 for v in fp.VARIANTS)
    assert all(fp.BY_NAME["fit_fallback"].params(v).k + 10 > 63 for v in fp.VARIANTS)
    for variant in fp.VARIANTS:
        c = fp.BY_NAME["rsvd_full_width"].params(variant)
        assert c.k + 10 >= min(c.n, c.p)


def test_the_drivers_reserve_leaves_room_for_the_null_mode_repair():
    """fix_null_columns runs when rsvd_core's panels are the only live part of the drivers' reserve (eofx_abi.hip: rsvd_finish
    repairs before it exports) and skips the repair without room.  What rsvd_scratch_bytes holds beyond those panels -- the
    export staging, the Gram partials, the split-K partials and the 4 MiB slack, none of them in use at that point -- covers
    null_repair_bytes of the longer factor at every shape: the "no room" branch is not a matter of what ran before.  (The
    repairs of the two factors follow each other inside a scope of their own, so the longer one is the requirement.)"""
    lib = plans_shim.lib()
    up = lambda x, m: (x + m - 1) // m * m          # noqa: E731
    shapes = [(64, 40000), (48, 30000), (64, 5000), (300, 2000), (2000, 300), (1000, 1000), (33, 1000000), (8000, 129600), (5, 7)]
    for n, p in shapes:
        tall_pad, small_pad = up(max(n, p), 512), up(min(n, p), 512)
        for k in (1, 8, 33, 40, 64, 200, 246):
            if k > min(n, p):
                continue
            l = min(k + 10, min(n, p))
            L, Lo = up(l, 32), up(k, 32)
            live = 4 * (2 * small_pad * L + 2 * tall_pad * L + tall_pad * Lo + small_pad * Lo) + 8 * (3 * L * L + 2 * L * Lo)
            live += 16 * 256 + (1 << 20)            # every carve rounds up to 256 bytes; 1 MiB for the small buffers of the scopes inside
            room = lib.pl_rsvd_scratch_bytes(tall_pad, small_pad, l, k) - live
            assert room >= lib.pl_null_repair_bytes(tall_pad, Lo), (n, p, k, room, lib.pl_null_repair_bytes(tall_pad, Lo))


def test_the_cross_probes_plan_both_routes():
    """the Gram route is taken when both fields are wider than long (eofx_plans.hpp, cross_plan): n < p1 and n < p2"""
    for name, gram in (("cross_gram_route", True), ("cross_plain_route", False), ("cross_sharded", True)):
        for variant in fp.VARIANTS:
            c = fp.BY_NAME[name].params(variant)
            assert (c.n < c.p1 and c.n < c.p2) == gram, (name, variant)
    c = fp.BY_NAME["cross_gram_route"].params("main")
    assert (c.n, c.p1, c.p2, c.k) == (300, 1300, 900, 6)


def test_null_mode_field_has_exactly_its_rank_in_float64():
    """64 x 40 000 of rank 3, k = 40: Lo = 64, so the repair's copy of the long factor alone is 10 MB -- above the 4 MiB slack of the
    drivers' reserve -- and exactly min(r, k) singular values stand above 1e-4 of the leading one"""
    lib = plans_shim.lib()
    for name in ("null_rsvd", "null_fit"):
        for variant in fp.VARIANTS:
            p = fp.BY_NAME[name]
            c = p.params(variant)
            se = fp.null_singular_values(c, fp.Gen(name, variant))
            assert int((se > 1e-4 * se[0]).sum()) == min(c.r, c.k) == c.r, (name, variant, se[:5])
            assert se[c.r] <= 1e-6 * se[0]          # (the float32 rounding of the field: a hundred times below the threshold)
            rows_pad = (c.p + 511) // 512 * 512
            assert rows_pad * 64 * 4 > (4 << 20) and lib.pl_null_repair_bytes(rows_pad, 64) > (4 << 20)
    c = fp.BY_NAME["null_rsvd"].params("main")
    assert (c.n, c.p, c.r, c.k) == (64, 40000, 3, 40)


def test_no_field_is_large():
    for p in fp.PROBES:
        for variant in fp.VARIANTS:
            c = p.cfg[variant]
            pairs = [(c[a], c[b]) for a, b in (("n", "p"), ("n", "p1"), ("n", "p2"), ("rows", "L"), ("rows_pad", "L")) if a in c and b in c]
            pairs += list(c.get("shapes", ()))
            assert all(4 * a * b <= 12.5e6 for a, b in pairs), (p.name, variant)
