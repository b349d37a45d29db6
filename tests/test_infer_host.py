"""Host-side checks of the row-invariant inference forward (no GPU): the bpenhance key, the exact-arithmetic data of
tests/test_infer_gpu.py, where the bp_infer_* kernels live in the built library, and that every one of them is reached by a named
case of tests/test_infer_gpu.py (the restatement of the dispatch is tests/infer_np.py).  Kernels are listed by name only
(llvm-objdump --offloading, --syms, the .kd symbols), as tests/test_dispatch_coverage.py does.  The same listing holds the build to
its rule: one shared library, one translation unit per subsystem (UNITS of csrc/Makefile), one gfx950 code object per unit."""
import os
import re
import shutil
import subprocess

import pytest

import dispatch_np as D
import infer_np as IN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
LIB = os.path.join(PKG, "libbp_hip.so")
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def _units():
    """The names on the UNITS line of csrc/Makefile."""
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    return re.search(r"^UNITS\s*=\s*(.+)$", mk, re.M).group(1).split()


def test_bpenhance_rejects_an_unknown_forward_without_a_device():
    exe = os.path.join(PKG, "bpenhance")
    if not os.path.exists(exe):
        pytest.fail("%s is not built (python __graft_entry__.py)" % exe)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, "forward=bogus"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "forward: bogus is not default or rowinv", (r.returncode, r.stdout, r.stderr)
    # the key is read with the others: a good value gets as far as the next check, still without a device
    r = subprocess.run([exe, "forward=rowinv"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.startswith("bpenhance: need layersizes"), r.stdout
    r = subprocess.run([exe, "forward=rowinv", "compute=bf16", "layersizes=264,96,33", "fea_dim=33", "fea_context=7", "targ_offset=3",
                        "norm_file=x", "initwts_file=y", "in_wav=a", "out_wav=b"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "bpenhance: forward=rowinv needs compute=fp32", r.stdout
    r = subprocess.run([exe, "method=logmmse", "fea_dim=129", "in_wav=a", "out_wav=b", "forward=rowinv"], capture_output=True, text=True,
                       timeout=60, env=env)
    assert r.returncode == 0 and "method=logmmse takes no forward" in r.stdout, r.stdout


@pytest.mark.parametrize("net", ["S", "W", "M"])
def test_exact_data_conditions(net):
    """Conditions (a) and (c) of tests/exact_data.py on the forward GEMMs of the data tests/test_infer_gpu.py::test_exact runs."""
    ls = {"S": IN.NET_S, "W": IN.NET_W, "M": IN.NET_M}[net]
    W, b = IN.exact_net(ls, 1)
    fails, fig = IN.exact_conditions(ls, W, b, IN.exact_inputs(ls, 65, 1))
    print(net, fig)
    assert not fails, fails
    assert fig["max_over_q_log2"] < 24


def test_the_plan_depends_on_the_shape_alone():
    """What the GPU tests rely on: S has no k-slices, every layer of W has 8, and no plan leaves k-rows out or takes one twice."""
    assert [IN.plan(320, 128), IN.plan(128, 64)] == [(1, 1, 5), (1, 1, 2)]
    assert [IN.plan(1600, 2048), IN.plan(2048, 2048), IN.plan(2048, 192)] == [(16, 8, 4), (16, 8, 4), (2, 8, 4)]
    assert [IN.plan(1024, 4096), IN.plan(4096, 576), IN.plan(576, 192)] == [(32, 4, 4), (5, 8, 8), (2, 2, 5)]      # net M
    for K in range(64, 8192 + 64, 64):
        for N in (64, 128, 192, 2048, 8192):
            tiles_n, splitk, per = IN.plan(K, N)
            assert splitk in (1, 2, 4, 8) and 4 * splitk * per >= K // IN.KU and (splitk == 1 or tiles_n * splitk <= 128)
    # the header restated: the same constants and the same loop
    src = open(os.path.join(PKG, "csrc", "bp_infer.h")).read()
    assert re.search(r"INFER_BM = %d, INFER_BN = %d, INFER_KU = %d, INFER_MAX_SPLITK = %d;" % (IN.BM, IN.BN, IN.KU, IN.MAX_SPLITK), src)
    assert "p.tiles_n * p.splitk * 2 <= 128 && U / (4 * p.splitk * 2) >= 3" in src


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
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
    return out


def test_infer_kernels_live_in_a_code_object_of_their_own(code_objects):
    assert len(code_objects) == len(_units()), "one gfx950 code object per unit of %s: %d" % (_units(), len(code_objects))
    holders = [names for names in code_objects if any("bp_infer_" in n for n in names)]
    assert len(holders) == 1, holders
    assert all("bp_infer_" in n for n in holders[0]), "bp_infer.hip's code object holds other kernels: %s" % sorted(holders[0])
    assert not any(D.family(n) for n in holders[0]), "a kernel of the six GEMM families in bp_infer.hip's code object"


def test_every_infer_kernel_is_reached_by_a_named_case(code_objects):
    kernels = set(n for names in code_objects for n in names if "bp_infer_" in n)
    claims = IN.case_claims()
    reached = set(c for v in claims.values() for c in v if " | " not in c)
    assert reached == kernels, "library %s, cases %s" % (sorted(kernels), sorted(reached))
    # ... and every branch the restatement names is taken by one of them, with both kernels where both can take it
    branches = set(c.split(" | ")[1] for v in claims.values() for c in v if " | " in c)
    assert branches == {"whole column tiles", "last column tile half empty", "even partial sums", "uneven partial sums",
                        "partial sums without k-rows", "1 k-slices", "2 k-slices", "4 k-slices", "8 k-slices",
                        "layers with different slice counts", "one row tile", "several row tiles", "row tile ends inside",
                        "whole row tiles"}, sorted(branches)
    # every slice count the plan can give (test_the_plan_depends_on_the_shape_alone) runs the k-split kernel's read-back
    split = IN.kernel(2048, 2048)
    assert all(any(c == "%s | %d k-slices" % (split, k) for v in claims.values() for c in v) for k in (2, 4, 8))
    gpu = open(os.path.join(ROOT, "tests", "test_infer_gpu.py")).read()
    for case in claims:
        name, tag = re.match(r"(\w+)\[(\w+)\]", case).groups()
        assert "def %s(" % name in gpu and '"%s' % tag in gpu, case



# Which unit's code object holds a kernel, by the kernel's name; the first row that matches.  A new subsystem adds its row.
UNIT_OF_KERNEL = [
    (r"bp_rbm_", "bp_rbm"),
    (r"bp_rir_|bp_mix_reverb_", "bp_room"),
    (r"bp_wave_resample$", "bp_resample"),
    (r"bp_mix_", "bp_mix"),                                # ... the other bp_mix_* kernels, with bp_mix_gain
    (r"bp_wave_", "bp_wave"),                              # ... the other bp_wave_* kernels, with bp_wave_analysis
    (r"bp_infer_", "bp_infer"),
    (r"bp_eval_", "bp_eval"),
    (r"bp_stream_", "bp_stream"),
    (r"bp_lmstream_|bp_logmmse_", "bp_classic"),
    (r"bp_dp_", "bp_dp"),
    (r"bp_peak_", "bp_profile"),
    (r"bp_gemm|bp_wgrad_dma|bp_(apply_mask|bias_bf16|fill_normal|out_split_stage|stage_bunch|to_bf16_both)$", "bp_step"),
]


def _unit_of(kernel):
    base = re.search(r"\bbp_\w+", kernel).group(0)         # the name without return type, template and argument lists
    for pat, unit in UNIT_OF_KERNEL:
        if re.match(pat, base):
            return unit
    pytest.fail("kernel %s matches no row of UNIT_OF_KERNEL: say which unit holds it" % kernel)


def test_every_kernel_lives_in_the_code_object_of_its_unit(code_objects):
    seen = {}
    for i, names in enumerate(code_objects):
        for n in names:
            assert n not in seen, "%s occurs in two code objects" % n
            seen[n] = i
    holder = {}                                            # unit -> the code objects that hold its kernels
    for n, i in seen.items():
        holder.setdefault(_unit_of(n), set()).add(i)
    assert sorted(holder) == sorted(_units()), "the units of the table against UNITS of the Makefile"
    assert all(len(v) == 1 for v in holder.values()), "a unit's kernels in more than one code object: %s" % holder
    assert len(set(min(v) for v in holder.values())) == len(holder), "two units share a code object: %s" % holder
    assert holder["bp_mix"] == {seen[n] for n in seen if n.startswith("bp_mix_gain(")}
    assert holder["bp_wave"] == {seen[n] for n in seen if n.startswith("bp_wave_analysis(")}


def test_one_library_defines_the_whole_abi():
    import dnnse_amd
    dyn = subprocess.check_output([READELF, "-d", LIB], universal_newlines=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.+?)\]", dyn)
    assert needed and not [n for n in needed if "bp_rbm" in n or "libbp_" in n], needed
    syms = subprocess.check_output([READELF, "--dyn-syms", "-W", LIB], universal_newlines=True)
    rows = [line.split() for line in syms.splitlines() if re.match(r"\s*\d+:", line)]
    defined = [r for r in rows if len(r) >= 8 and r[6] != "UND"]          # Num Value Size Type Bind Vis Ndx Name
    names = set(r[7].split("@")[0] for r in defined)
    missing = [s for s in dnnse_amd.ABI_SYMBOLS if s not in names]
    assert not missing, "not defined in libbp_hip.so itself: %s" % missing
    err = [r[7] for r in defined if r[3] == "TLS" and "g_bp_err" in r[7]]
    assert len(err) == 1, "the thread's error string is defined %d times: %s" % (len(err), err)
    assert not [r[7] for r in rows if "g_bp_err" in r[-1] and r[3] == "TLS" and r[6] == "UND"]
