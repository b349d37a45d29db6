"""The pre-training entry points without a GPU (the bp_rbm_* block of include/bp_c_api.h): the defaults, every argument check of
bp_rbm_create and bp_rbm_set_hyper (they answer before the device is touched, so they answer here), the ctypes structs against the
header, the restatement's own identities, and the mutant table of tests/rbm_np.py: nine wrong implementations, each shown from the
restatement alone to miss the bar of the check that tests/test_rbm_gpu.py holds the device to by at least MUTANT_FACTOR."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rbm_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BP_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _err(lib):
    return lib.bp_last_error().decode()


# ------------------------------------------------------------------ defaults
def test_defaults_are_the_table_of_the_header(pkg, lib):
    d1, d2, d5 = pkg.rbm_defaults(1), pkg.rbm_defaults(2), pkg.rbm_defaults(5)
    f32 = lambda v: float(np.float32(v))
    assert d1 == dict(lrate=f32(0.0005), momentum=f32(0.9), weightcost=f32(1e-5), visible=0, sample=1)
    assert d2 == dict(lrate=f32(0.01), momentum=f32(0.9), weightcost=f32(1e-5), visible=1, sample=1) and d5 == d2
    assert lib.bp_rbm_defaults(1, None) == BP_ERR_ARG and lib.bp_rbm_defaults(0, C.byref(pkg.BPRbmHyper())) == BP_ERR_ARG
    assert lib.bp_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()
    for name in pkg.ABI_SYMBOLS:
        if name.startswith("bp_rbm_"):
            assert re.search(r"\bint %s\(" % name, hdr), name
            assert hasattr(lib, name)
    assert sorted(n for n in pkg.ABI_SYMBOLS if n.startswith("bp_rbm_")) == sorted(set(re.findall(r"\bint (bp_rbm_\w+)\(", hdr)))


# ------------------------------------------------------------------ argument checks, all before the device
def _create_args(pkg, sizes=(6, 4, 3), bunch=4, cap=16, device=0):
    cfg = pkg.BPRbmConfig()
    cfg.device, cfg.numlayers, cfg.bunchsize, cfg.max_chunk_frames, cfg.seed = device, len(sizes), bunch, cap, 1
    for i, s in enumerate(sizes[:pkg.MAXLAYER]):
        cfg.layersizes[i] = s
    P = C.POINTER(C.c_float)
    keep, w, c = [], (P * pkg.MAXLAYER)(), (P * pkg.MAXLAYER)()
    for l in range(1, min(len(sizes), pkg.MAXLAYER)):
        for arr, n in ((w, max(sizes[l - 1], 1) * max(sizes[l], 1)), (c, max(sizes[l], 1))):
            a = np.zeros(n, np.float32)
            keep.append(a)
            arr[l] = a.ctypes.data_as(P)
    return cfg, w, c, keep


CREATE_CASES = [
    ("numlayers_one", dict(sizes=(6,)), "numlayers"), ("numlayers_eleven", dict(sizes=(4,) * 10, numlayers=11), "numlayers"),
    ("size_zero", dict(sizes=(6, 0, 3)), "layer size"), ("size_negative", dict(sizes=(6, 4, -3)), "layer size"),
    ("bunch_zero", dict(bunch=0), "bunchsize"), ("bunch_negative", dict(bunch=-4), "bunchsize"),
    ("capacity_negative", dict(cap=-1), "max_chunk_frames"), ("device_negative", dict(device=-1), "device"),
]


@pytest.mark.parametrize("name,kw,needle", CREATE_CASES, ids=[c[0] for c in CREATE_CASES])
def test_create_refuses_bad_configurations(pkg, lib, name, kw, needle):
    kw = dict(kw)
    numlayers = kw.pop("numlayers", None)
    cfg, w, c, keep = _create_args(pkg, **kw)
    if numlayers is not None:
        cfg.numlayers = numlayers
    out = C.c_void_p()
    assert lib.bp_rbm_create(C.byref(cfg), w, c, None, C.byref(out)) == BP_ERR_ARG
    assert needle in _err(lib) and not out.value


def test_create_refuses_null_pointers(pkg, lib):
    cfg, w, c, keep = _create_args(pkg)
    out = C.c_void_p()
    for args in ((None, w, c, None, C.byref(out)), (C.byref(cfg), None, c, None, C.byref(out)), (C.byref(cfg), w, None, None, C.byref(out)),
                 (C.byref(cfg), w, c, None, None)):
        assert lib.bp_rbm_create(*args) == BP_ERR_ARG and "null" in _err(lib)
    P = C.POINTER(C.c_float)
    for which in (0, 1):
        cfg, w, c, keep = _create_args(pkg)
        (w, c)[which][2] = P()
        assert lib.bp_rbm_create(C.byref(cfg), w, c, None, C.byref(out)) == BP_ERR_ARG and "null" in _err(lib)
    assert not out.value


HYPER_CASES = [
    ("lrate_negative", dict(lrate=-0.1), "lrate"), ("lrate_nan", dict(lrate=float("nan")), "lrate"), ("lrate_inf", dict(lrate=float("inf")), "lrate"),
    ("weightcost_negative", dict(weightcost=-1e-5), "weightcost"), ("weightcost_nan", dict(weightcost=float("nan")), "weightcost"),
    ("weightcost_inf", dict(weightcost=float("inf")), "weightcost"),
    ("momentum_one", dict(momentum=1.0), "momentum"), ("momentum_negative", dict(momentum=-0.1), "momentum"), ("momentum_nan", dict(momentum=float("nan")), "momentum"),
    ("visible_two", dict(visible=2), "visible"), ("visible_negative", dict(visible=-1), "visible"), ("sample_two", dict(sample=2), "sample"),
]


@pytest.mark.parametrize("name,kw,needle", HYPER_CASES, ids=[c[0] for c in HYPER_CASES])
def test_set_hyper_refuses_bad_values_before_it_looks_at_the_stack(pkg, lib, name, kw, needle):
    """The values are checked first, so the refusal can be seen without a stack (and so without a device): the message names the value."""
    f = dict(pkg.rbm_defaults(1), **kw)
    h = pkg.BPRbmHyper(f["lrate"], f["momentum"], f["weightcost"], f["visible"], f["sample"])
    assert lib.bp_rbm_set_hyper(None, 1, C.byref(h)) == BP_ERR_ARG
    assert needle in _err(lib) and "null stack" not in _err(lib)


def test_null_stack_and_null_hyper_are_refused(pkg, lib):
    f = pkg.rbm_defaults(1)
    h = pkg.BPRbmHyper(f["lrate"], f["momentum"], f["weightcost"], f["visible"], f["sample"])
    assert lib.bp_rbm_set_hyper(None, 1, C.byref(h)) == BP_ERR_ARG and "null stack" in _err(lib)
    assert lib.bp_rbm_set_hyper(None, 1, None) == BP_ERR_ARG and "null hyper" in _err(lib)
    x = np.zeros(8, np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.bp_rbm_train_chunk(None, 1, 1, fp, None) == BP_ERR_ARG
    assert lib.bp_rbm_up(None, 1, 1, fp, fp) == BP_ERR_ARG
    assert lib.bp_rbm_step(None, 1, fp, 0, None) == BP_ERR_ARG
    assert lib.bp_rbm_steps(None, 1, C.byref(C.c_uint())) == BP_ERR_ARG
    assert lib.bp_rbm_get(None, None, None, None) == BP_ERR_ARG
    assert lib.bp_rbm_destroy(None) == 0


# ------------------------------------------------------------------ the structs
def _header_fields(struct):
    hdr = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(int|float|double|uint64_t)\s+", "", decl.strip())
        names += [re.sub(r"\[.*\]", "", n).strip().lstrip("*") for n in decl.split(",") if n.strip()]
    return names


def test_structs_match_the_header(pkg):
    assert _header_fields("bp_rbm_config") == [f[0] for f in pkg.BPRbmConfig._fields_]
    assert _header_fields("bp_rbm_hyper") == [f[0] for f in pkg.BPRbmHyper._fields_]
    assert _header_fields("bp_rbm_trace") == [f[0] for f in pkg.BPRbmTrace._fields_]
    assert C.sizeof(pkg.BPRbmConfig) == 4 * (2 + pkg.MAXLAYER + 2) + 8 and C.sizeof(pkg.BPRbmHyper) == 20 and C.sizeof(pkg.BPRbmTrace) == 72


# ------------------------------------------------------------------ the restatement's own identities
def test_uniforms_are_exact_fp32_numbers_in_the_unit_interval():
    u = R.uniforms(R.SEED, 3, 2, 24, 33)
    assert u.dtype == np.float32 and u.shape == (24, 33) and u.min() >= 0.0 and u.max() < 1.0
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.floor(k)) and k.max() < 2 ** 24
    # the keying is the dropout mask's (philox_np.drop_mask): u < p on the top 24 bits against word < p 2^32 can differ only in the
    # low 8 bits; at p = 1/2 they agree exactly
    import philox_np as P
    assert np.array_equal((u < np.float32(0.5)).astype(np.uint8), P.drop_mask(R.SEED, 3, 2, 24, 33, 0.5))
    assert not np.array_equal(u, R.uniforms(R.SEED + 1, 3, 2, 24, 33)) and not np.array_equal(u, R.uniforms(R.SEED, 4, 2, 24, 33))


@pytest.mark.parametrize("sid", list(R.STACKS))
def test_the_stacked_form_of_the_statistics_is_the_difference_of_the_two_products(sid):
    st = R.STACKS[sid]
    B, H = st.bunch, st.sizes[1]
    W, c, a = (x[1] for x in R.params(st))
    r = R.cd1(R.rows(st)[:B], W, c, a, 0, True, R.uniforms(R.SEED, 0, 1, B, H))
    Bp = R.pad64(B)
    Xs, Ps = np.zeros((2 * Bp, st.sizes[0])), np.zeros((2 * Bp, H))
    Xs[:B], Xs[Bp:Bp + B], Ps[:B], Ps[Bp:Bp + B] = r["v0"], r["v1"], -r["p0"], r["p1"]
    assert R.relmax(Xs.T @ Ps, r["gw"], np.abs(r["pos"]).max()) < 1e-14
    assert R.relmax(Ps.sum(0), r["gc"], r["p0"].sum(0).max()) < 1e-14
    # the first two mutants are visible only where gW is not small beside the positive statistic
    assert np.abs(r["gw"]).max() >= 0.05 * np.abs(r["pos"]).max()
    assert set(np.unique(r["s0"])) <= {0.0, 1.0} and 0.2 < r["s0"].mean() < 0.8


def test_the_unmutated_restatement_is_inside_every_bar():
    for sid in ("S", "W"):
        st = R.STACKS[sid]
        B, H = st.bunch, st.sizes[1]
        W, c, a = (x[1] for x in R.params(st))
        u = R.uniforms(R.SEED, 0, 1, B, H)
        r = R.cd1(R.rows(st)[:B], W, c, a, 0, True, u)
        e = R.stage_errors(R._as_trace(r), W, c, a, 0, True, u)
        assert max(e.values()) < 1.0, e          # fp32 storage of float64 values: far inside


# ------------------------------------------------------------------ the mutants
MUTANT_RUNS = [(m, "B" if m == "pad_columns_at_half" else h) for m in R.MUTANTS for h in (("A", "B") if R.CAUGHT_BY[m] in "Wca" else ("A",))]


@pytest.mark.parametrize("name,hset", MUTANT_RUNS, ids=["%s-%s" % r for r in MUTANT_RUNS])
def test_every_mutant_misses_its_bar_by_the_factor(name, hset):
    stack = "W" if name == "bernoulli_visibles_left_linear" else "S"
    m = R.miss(name, stack, hset)
    print("%s (%s, set %s): %.3g bars" % (name, R.CAUGHT_BY[name], hset, m))
    assert m >= R.MUTANT_FACTOR, (name, m)


def test_the_table_names_nine_mutants_and_a_check_for_each():
    assert len(R.MUTANTS) == 9 and set(R.CAUGHT_BY) == set(R.MUTANTS)
    assert set(R.CAUGHT_BY.values()) <= {"gw", "v1", "W", "c", "a"}
    assert R.HYPER["A"] == R.Hyper(0.002, 0.5, 1.0 / 16) and R.HYPER["B"] == R.Hyper(0.05, 0.9, 1.0 / 64)
    assert (R.GEMM_BAR, R.UPDATE_BAR, R.RECON_BAR, R.TEN_STEP_BAR) == (1e-4, 1e-5, 1e-9, 1e-4)
    assert [(s.sizes, s.bunch) for s in R.STACKS.values()] == [((70, 33, 20), 24), ((264, 200, 136), 64), ((520, 300), 128), ((70, 33, 20), 40)]
