"""Every GEMM-family kernel the library ships has faced the oracle -- checked without a GPU.

The kernels are listed from the BUILT library's gfx950 code objects (llvm-objdump --offloading, --syms on what that extracts, the
.kd symbols, c++filt; nothing is compiled here).  tests/dispatch_np.py restates which of them a configuration launches,
tests/dispatch_cases.py is the matrix that tests/test_dispatch_gpu.py runs, and profiles/r07_dispatch_kernels.txt holds the
distinct kernel names of one run of that file under a kernel trace.  A new template instantiation, a renamed template parameter
or a dropped case fails here and the message names the kernel."""
import itertools
import os
import shutil
import subprocess

import pytest

import dispatch_cases as DC
import dispatch_np as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "libbp_hip.so")
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
TRACE = os.path.join(ROOT, "profiles", "r07_dispatch_kernels.txt")

# Kernels of the six families that no case of the matrix claims, each with the reason.  Empty: a pull request that adds an
# instantiation adds a case.
UNCLAIMED = {}

# The small kernels of bp_step.hip's code object do not depend on the shape of the net; the existing test that covers each:
SMALL_KERNELS = {
    "bp_stage_bunch": "tests/test_gpu_parity.py::test_window_chunk_equals_stacked_chunk (window chunks), ::test_train_matches_oracle (visible dropout)",
    "bp_apply_mask": "tests/test_gpu_parity.py::test_golden_dropout_training_with_injected_masks",
    "bp_fill_normal": "tests/test_gpu_parity.py::test_two_runs_of_many_steps_agree_bit_for_bit (fill_chunk_synthetic)",
    "bp_to_bf16_both": "tests/test_gpu_parity.py::test_bf16_step_matches_bf16_oracle",
    "bp_bias_bf16": "tests/test_gpu_parity.py::test_bf16_step_matches_bf16_oracle (bunch sizes outside the LDS-DMA set)",
}


def _short(name):
    """bp_stage_bunch for `bp_stage_bunch(StageArgs)`."""
    return name.replace("void ", "").split("<", 1)[0].split("(", 1)[0]


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """[set of demangled kernel names] per gfx950 code object of the library (one per translation unit)."""
    if not os.path.exists(LIB):
        pytest.fail("%s is not built (python __graft_entry__.py)" % LIB)
    if not os.path.exists(OBJDUMP) or not shutil.which("c++filt"):
        pytest.fail("llvm-objdump / c++filt not found")
    tmp = str(tmp_path_factory.mktemp("offload"))
    shutil.copy(LIB, os.path.join(tmp, "lib.so"))
    subprocess.check_call([OBJDUMP, "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL)
    out = []
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        syms = subprocess.check_output([OBJDUMP, "--syms", f], cwd=tmp, universal_newlines=True)
        mangled = [line.split()[-1][:-3] for line in syms.splitlines() if line.strip().endswith(".kd")]
        names = subprocess.check_output(["c++filt"], input="\n".join(mangled) + "\n", universal_newlines=True).split("\n")
        out.append(set(n.strip() for n in names if n.strip()))
    shutil.rmtree(tmp, ignore_errors=True)
    assert out, "no gfx950 code object in " + LIB
    return out


@pytest.fixture(scope="module")
def shipped(code_objects):
    """The six families' kernels; they all live in one code object (bp_step.hip's)."""
    holders = [names for names in code_objects if any(D.family(n) for n in names)]
    assert len(holders) == 1, "kernels of the six GEMM families in %d code objects: only bp_step.hip launches them, and " \
        "tests/dispatch_np.py restates only its dispatch: %s" % (len(holders), [sorted(n for n in h if D.family(n)) for h in holders[1:]])
    return set(n for n in holders[0] if D.family(n)), set(n for n in holders[0] if not D.family(n))


def _claims():
    return {c.id: D.case_paths(c.ls, c.B, c.dtype, 1 if c.out else 0) for c in DC.CASES}


def test_library_ships_fifty_kernels_in_six_families(shipped):
    kernels, small = shipped
    per = {}
    for n in kernels:
        per[D.family(n)] = per.get(D.family(n), 0) + 1
    assert per == {"bp_gemm": 7, "bp_gemm_multi": 5, "bp_out_split_stage": 2, "bp_wgrad_dma": 6, "bp_gemm_bf16": 22,
                   "bp_wgrad_dma_bf16_six": 4, "bp_wgrad_dma_bf16_store": 4}, per
    assert set(_short(n) for n in small) == set(SMALL_KERNELS), \
        "small kernels of bp_step.hip changed: list each in SMALL_KERNELS with the test that covers it"


def test_every_name_of_the_restatement_exists_in_the_library(shipped):
    """A sweep over widths, bunch sizes, depths, both dtypes and both output layers: whatever name the restatement returns is
    a kernel of the library (a renamed or re-ordered template parameter fails here, with the name)."""
    kernels, _ = shipped
    widths = [33, 64, 130, 257, 514, 600, 1000, 1024, 2048, 2100, 6600]
    bunches = [1, 12, 64, 100, 128, 200, 256, 300, 512, 1000, 1040, 2048]
    seen = set()
    for B, dtype, logi in itertools.product(bunches, (0, 1), (0, 1)):
        for ls in itertools.chain(itertools.product(widths, repeat=2), itertools.product(widths[::2], repeat=3), [DC.NINE]):
            for call in ("step", "grads", "forward"):
                seen |= D.kernels(list(ls), B, dtype, logi, call)
    for c in DC.CASES:
        seen |= D.case_kernels(c.ls, c.B, c.dtype, 1 if c.out else 0)
    assert not seen - kernels, "the restatement names kernels the library does not hold: %s" % sorted(seen - kernels)
    assert seen == kernels, "kernels no swept configuration reaches (restatement out of date?): %s" % sorted(kernels - seen)


def test_every_kernel_is_claimed_by_a_case_of_the_matrix(shipped):
    kernels, _ = shipped
    claimed = set().union(*_claims().values())
    assert not set(UNCLAIMED) - kernels, "UNCLAIMED lists kernels the library does not hold"
    missing = kernels - claimed - set(UNCLAIMED)
    assert not missing, "kernels that no case of tests/dispatch_cases.py reaches (add a case): %s" % sorted(missing)
    assert not UNCLAIMED, "the allowlist is empty for the six families"


def test_every_case_claims_something_no_other_case_does():
    """Kernels, tile-map branches, a second grouped launch, or tiles that end inside the matrix: dropping a case loses one."""
    claims = _claims()
    for cid, mine in claims.items():
        others = set().union(*[v for k, v in claims.items() if k != cid])
        assert mine - others, "case %s reaches nothing the other cases do not" % cid


def test_tile_map_branches_and_edge_tiles(shipped):
    """Every fp32 tile configuration runs with an n-tile count that is a multiple of 8 and with one that is not (the two branches
    of the XCD tile map), and every tile size once with widths that are no multiples of 64 at a bunch that is no multiple of 32."""
    kernels, _ = shipped
    claimed = set().union(*_claims().values())
    configs = set(D.tile_config(n) for n in kernels)
    for cf in sorted(configs):
        if cf.startswith("GemmKernel<"):
            for branch in ("xcd map", "plain map"):
                assert "%s | %s" % (cf, branch) in claimed, "no case runs %s with the %s" % (cf, branch)
        if cf != "bp_wgrad_dma":                                # (its bunch sizes are 128 / 256 / 512 exactly)
            assert "%s | ragged" % cf in claimed, "no case runs %s with every edge inside a tile" % cf
    for grouped in (D.n_multi(64, 64, 32, 2, 2, False, False, D.EPI_WGRAD_UPDATE), D.n_multi(128, 64, 16, 2, 2, False, False, D.EPI_WGRAD_STORE),
                    D.n_wgrad_dma(128, False)):
        assert grouped + " | group 2" in claimed, "no case reaches the second group of four of " + grouped


def test_the_hardware_launched_what_the_restatement_says(shipped):
    """profiles/r07_dispatch_kernels.txt: the distinct kernel names of tests/test_dispatch_gpu.py under a kernel trace.  Restricted
    to the six families it equals the union of the restatement over the matrix, which is everything the library ships."""
    kernels, _ = shipped
    traced = set()
    for line in open(TRACE):
        n = line.strip()
        if n.endswith(".kd"):
            n = n[:-3]
        if n and not n.startswith("#") and D.family(n):
            traced.add(n)
    union = set().union(*[D.case_kernels(c.ls, c.B, c.dtype, 1 if c.out else 0) for c in DC.CASES])
    assert traced == union, "traced but not predicted: %s; predicted but not traced: %s" % (sorted(traced - union), sorted(union - traced))
    assert union == kernels, sorted(kernels - union)
    assert len(traced) == 50


def test_spreads_of_the_table_pick_the_bars():
    """The spread figures next to the cases (dispatch_cases.py): every fp32 case that has an oracle supports the 1e-5 bar on its
    one-bunch gradient, by the table and by the CPU oracle run here on the cheap ones."""
    for c in DC.CASES:
        assert (c.out is None) == (c.spread is not None), c.id
        if c.dtype == 0 and c.out is None:
            assert DC.strict_bar(c.spread), c.id
            if max(c.ls) * c.B <= 300 * 1024:
                assert DC.strict_bar(DC.oracle_spread(c)), (c.id, c.spread, DC.oracle_spread(c))
