"""Every frame size the signal layer accepts faces a reference through every entry point that takes one -- checked without a GPU.

tests/geometry_cases.py holds the six sizes and, per entry point and size, the id of the GPU test that does the comparison.  Here:
the library accepts exactly those six (probed through the two host-only counts calls), every cell names a test that its module
really defines with the gpu mark, and the sentence lengths of the resynthesis cases contain their edge lengths at every size.  A
seventh size, a dropped parametrize entry or a renamed test fails here and the message names the cell."""
import json
import os

import numpy as np
import pytest

import geometry_cases as GC
import wave_np as WN

ENTRY_POINTS = ["wave_lps", "enhance_waves lps", "enhance_waves mask", "stream_open", "stream_open rowinv", "mix_features",
                "score_waves", "logmmse_waves", "logmmse_stream_open", "eval_mix",
                # the entry points added after the table was first closed
                "logmmse_waves spp", "logmmse_stream_open spp", "enhance_waves dynamic", "mix_features dynamic", "stream_open dynamic",
                "train_mix dynamic", "wave_mfcc", "post_rows", "gv_mix raw", "gv_mix post", "enhance_waves post", "stream_open post"]


def _accepted(pkg, call):
    ok = []
    for D in range(2, 1101):
        try:
            call(D)
            ok.append(D)
        except pkg.BPError as e:
            assert "status -1" in str(e), (D, str(e))
    return ok


def test_the_library_accepts_exactly_the_six_sizes(pkg):
    assert GC.FEA_DIMS == [(1 << k) + 1 for k in range(5, 11)]
    assert _accepted(pkg, lambda D: pkg.stream_counts(D, 3, 1, True, 5 * D, False)) == GC.FEA_DIMS
    assert _accepted(pkg, lambda D: pkg.logmmse_stream_counts(D, 6, 5 * D, False)) == GC.FEA_DIMS


def test_every_cell_names_a_gpu_test_that_exists():
    assert list(GC.COVERAGE) == ENTRY_POINTS
    cells = [(entry, D, cell) for entry, row in GC.COVERAGE.items() for D, cell in row.items()]
    for entry, row in GC.COVERAGE.items():
        assert sorted(row) == GC.FEA_DIMS, "%s: a cell for each of %s, none left at 'never'" % (entry, GC.FEA_DIMS)
    cells += [(entry, D, cell) for entry, row in GC.EXTRA.items() for D, cell in row.items()]
    ids = {}
    for entry, D, cell in cells:
        path, test = cell.split("::")
        if path not in ids:
            ids[path] = GC.collected_ids(path)
        have, mod = ids[path]
        assert test in have, "%s at fea_dim %d: %s has no test %s" % (entry, D, path, test)
        fn = getattr(mod, test.split("[")[0])
        marks = getattr(mod, "pytestmark", [])
        marks = (marks if isinstance(marks, list) else [marks]) + list(getattr(fn, "pytestmark", []))
        assert any(m.name == "gpu" for m in marks), cell
        assert not any(m.name in ("skip", "skipif", "xfail") for m in marks), cell
    assert sorted(GC.STREAM_MASK) == [257, 1025] and GC.EXTRA["stream_open mask"] is GC.STREAM_MASK
    assert sorted(GC.EXTRA["stream_open dynamic rowinv"]) == [33, 1025] and sorted(GC.EXTRA["set_mix_aux"]) == [257]


def test_every_symbol_of_the_c_api_is_classified():
    """include/bp_c_api.h against geometry_cases.API: every prototype is mapped to the rows that hold it or to the reason it has
    no frame size, every row is named by a symbol, and a prototype that takes a fea_dim has rows unless it is host only.  An
    entry point added to the header fails here until it is classified."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    protos = GC.api_prototypes(open(os.path.join(root, "include", "bp_c_api.h")).read())
    assert len(protos) > 100 and "bp_enhance_waves" in protos and "bp_last_error" in protos
    missing, stale = sorted(set(protos) - set(GC.API)), sorted(set(GC.API) - set(protos))
    assert not missing, "include/bp_c_api.h declares %s: give each its COVERAGE rows or a reason in geometry_cases.API" % missing
    assert not stale, "geometry_cases.API names %s, which include/bp_c_api.h does not declare" % stale
    named = set()
    for sym, what in GC.API.items():
        if isinstance(what, tuple):
            assert what and all(r in GC.COVERAGE for r in what), "%s: %s holds no such row" % (sym, [r for r in what if r not in GC.COVERAGE])
            named |= set(what)
        else:
            assert isinstance(what, str) and what.strip(), sym
            assert "fea_dim" not in protos[sym] or what.startswith("host only"), "%s takes a fea_dim: name its rows" % sym
    assert named == set(GC.COVERAGE), "rows that no symbol names: %s" % sorted(set(GC.COVERAGE) - named)


def test_the_cells_of_one_test_carry_its_size():
    """A cell that names a parametrised size names its own column (no row points every size at the one case that exists)."""
    for entry, row in GC.COVERAGE.items():
        for D, cell in row.items():
            digits = [int(t) for t in "".join(c if c.isdigit() else " " for c in cell.split("::")[1].split("[")[-1]).split()]
            sized = [v for v in digits if v in GC.FEA_DIMS]
            assert not sized or sized == [D], (entry, D, cell)


@pytest.mark.parametrize("D", GC.FEA_DIMS)
def test_sentence_lengths_contain_the_edges(D):
    n_fft, hop = WN.geometry(D)
    lens = GC.lengths(D)
    assert lens == [1, hop - 1, hop, hop + 1, n_fft - 1, 5 * hop + 7, 12 * hop + 3]
    for what, n in GC.edge_lengths(D).items():
        assert n in lens, (D, what)
    frames = [WN.n_frames(n, D) for n in lens]
    assert min(frames) == 2 and any(f < 6 for f in frames) and max(frames) >= 6      # the NAT clamp and past it
    assert sum(frames) % GC.BUNCH != 0 and sum(frames) > 2 * GC.BUNCH                 # full bunches and a partial one
    assert sum(frames) < 50 and sum(lens) <= 41000
    xs = GC.sentences(D)
    assert [x.size for x in xs] == lens and all(x.dtype == np.float32 for x in xs)
    a, e = GC.silent_stretch(D)
    assert not xs[-1][a:e].any() and xs[-1][a - 1] != 0 and xs[-1][e] != 0 and all(x[0] != 0 for x in xs)
    zf = GC.zero_frames(WN.analysis(xs[-1], D))
    assert list(zf) == [4, 5, 6]                                # frame t covers samples [(t - 1) hop, (t + 1) hop)
    assert GC.zero_segment(D, zf) == (4 * hop, 6 * hop)
    assert all(len(GC.zero_frames(WN.analysis(x, D))) == 0 for x in xs[:-1])


def test_committed_numbers_hold_a_figure_below_its_bar_for_every_cell():
    """profiles/geometry_parity_numbers.json: `python tests/geometry_cases.py numbers <parity JSON>` behind a -m gpu run."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "geometry_parity_numbers.json")
    num = json.load(open(path))
    for entry, row in GC.COVERAGE.items():
        for D, cell in row.items():
            fig = GC.cell_figure(entry, D, num["tests"].get(cell))
            assert fig is not None, "no measured figure for %s" % cell
            text, value, bar = fig
            assert num["table"][entry][str(D)] == text
            assert value <= bar and np.isfinite(value), (cell, text)
    for row in GC.EXTRA.values():
        for cell in row.values():
            rec = num["tests"][cell]
            assert rec.get("samples_differing", rec.get("words_differing")) == 0, cell
