"""The frame sizes of the signal layer and, for every public entry point that takes a fea_dim, the GPU test that holds it to a
reference at each of them (tests/test_geometry_coverage.py checks without a GPU that every cell names a test that exists;
tests/test_geometry_gpu.py holds the cases that no older file had the body for).

What changes with the size (csrc/bp_fft.h): the trip counts of fft_lds / rfft_frame / synth_frame (less than one item per thread
at 33, five bins per thread at 1025), the padded LDS index and the dynamic LDS sizes, and the workgroups per sentence of the two
noise-aware-row kernels (kb = ceil(D / 256): one up to 129, two at 257, three at 513, five at 1025).

A cell is "tests/<file>.py::<test>[<id>]", the id as pytest prints it.  The stream cells compare bit for bit with the offline call
of the same size, which the `enhance_waves` rows hold to the float64 restatement; eval_mix compares bit for bit with its parts."""
import numpy as np

FEA_DIMS = [33, 65, 129, 257, 513, 1025]
WAVE_BAR = 1e-5            # analysis and resynthesis: of the largest magnitude (tests/test_wave_f32_host.py: 30 x an fp32 restatement)
CTX, TOFF, BUNCH, HIDDEN = 3, 1, 16, 64


def lengths(fea_dim):
    """The sentence lengths of the resynthesis cases: one sample, one sample either side of the hop, one short of a frame, a few
    frames, and a dozen frames (whose samples [3 hop, 7 hop) are silent)."""
    hop = fea_dim - 1
    return [1, hop - 1, hop, hop + 1, 2 * hop - 1, 5 * hop + 7, 12 * hop + 3]


def edge_lengths(fea_dim):
    """What lengths() must contain at every size."""
    hop = fea_dim - 1
    return {"one sample": 1, "hop - 1": hop - 1, "hop": hop, "hop + 1": hop + 1, "n_fft - 1": 2 * hop - 1}


def silent_stretch(fea_dim):
    hop = fea_dim - 1
    return 3 * hop, 7 * hop


def sentences(fea_dim):
    """PCM16-like noise of the lengths above (seeded by the size); the last sentence with its silent stretch."""
    import wave_np as WN
    xs = WN.make_sentences(np.random.default_rng(1000 + fea_dim), lengths(fea_dim))
    a, e = silent_stretch(fea_dim)
    xs[-1][a:e] = 0.0
    return xs


def zero_frames(Y):
    """Frames of a restated spectrum whose every bin is exactly zero."""
    return np.flatnonzero((np.abs(Y) == 0.0).all(axis=1))


def zero_segment(fea_dim, frames):
    """Samples of the sentence that only all-zero frames cover: frames t and t + 1 cover [t hop, (t + 1) hop)."""
    hop = fea_dim - 1
    pairs = [t for t in frames if t + 1 in set(frames)]
    return (min(pairs) * hop, (max(pairs) + 1) * hop) if pairs else None


def net_sizes(fea_dim, target):
    """[(ctx + 1) D, 64, out]: out = D for the LPS target; the mask target reads the upper block of a [LPS | mask] output layer."""
    return [(CTX + 1) * fea_dim, HIDDEN, fea_dim if target == "lps" else 2 * fea_dim]


def _per_size(fmt, sizes=FEA_DIMS):
    return {D: fmt % D for D in sizes}


def _merge(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


GEO = "tests/test_geometry_gpu.py::"
COVERAGE = {
    "wave_lps": _per_size("tests/test_wave_gpu.py::test_analysis_matches_numpy[%d]"),
    "enhance_waves lps": _per_size(GEO + "test_resynthesis_matches_restatement[lps-%d]"),
    "enhance_waves mask": _per_size(GEO + "test_resynthesis_matches_restatement[mask-%d]"),
    "stream_open": _merge({33: "tests/test_stream_gpu.py::test_any_chunking_same_bits[ragged]"},
                          _per_size("tests/test_stream_gpu.py::test_other_configurations[fea%d]", FEA_DIMS[1:])),
    "stream_open rowinv": _merge({33: "tests/test_infer_gpu.py::test_packed_stream_same_bits[3-ragged]"},
                                 _per_size("tests/test_stream_gpu.py::test_other_configurations[fea%d_packed]", FEA_DIMS[1:])),
    "mix_features": _per_size("tests/test_mix_gpu.py::test_features_match_restatement[%d]"),
    "score_waves": _merge(_per_size("tests/test_eval_gpu.py::test_score_waves_match_restatement[%d-16000]", [129, 257]),
                          _per_size(GEO + "test_scores_match_restatement[%d]", [33, 65, 513, 1025])),
    "logmmse_waves": _merge(_per_size("tests/test_classic_gpu.py::test_waves_match_restatement[%d]", [33, 65, 129, 257]),
                            {D: "tests/test_classic_gpu.py::test_wide_spectrum_paths" for D in (513, 1025)}),
    "logmmse_stream_open": _merge({33: "tests/test_lmstream_gpu.py::test_any_chunking_same_bits[ragged17]"},
                                  _per_size("tests/test_lmstream_gpu.py::test_fixture_sentences[%d]", [65, 129, 257]),
                                  _per_size("tests/test_lmstream_gpu.py::test_wide_spectra[%d]", [513, 1025])),
    "eval_mix": _merge({129: "tests/test_eval_gpu.py::test_eval_mix_is_its_parts[0-False-False]"},
                       _per_size(GEO + "test_eval_mix_is_its_parts[%d]", [33, 65, 257, 513, 1025])),
}
# the mask target at an odd column offset of a padded output row (out_col = D), streamed
STREAM_MASK = _per_size("tests/test_stream_gpu.py::test_other_configurations[fea%d_mask]", [257, 1025])


def collected_ids(module_path):
    """Every id pytest would collect from the functions of a test module, from its parametrize marks alone (closest decorator
    first, as pytest joins them): {"test_x[a-b]", ...}; a test without parameters is its bare name."""
    import importlib
    import itertools
    mod = importlib.import_module(module_path[len("tests/"):-len(".py")])
    out = set()
    for name in dir(mod):
        fn = getattr(mod, name)
        if not name.startswith("test_") or not callable(fn):
            continue
        axes = []
        for m in getattr(fn, "pytestmark", []):
            if m.name != "parametrize":
                continue
            given = m.kwargs.get("ids")
            axes.append([str(given[k]) if given else _value_id(v) for k, v in enumerate(m.args[1])])
        out |= {"%s[%s]" % (name, "-".join(c)) for c in itertools.product(*axes)} if axes else {name}
    return out, mod


def _value_id(v):
    if isinstance(v, (tuple, list)):
        return "-".join(_value_id(x) for x in v)
    assert isinstance(v, (int, float, str, bool)), "geometry_cases.collected_ids: give %r an id" % (v,)
    return str(v)


# What a test's record says about its cell: (key, bar) pairs, the worst ratio is shown.  "bits": a bit-for-bit comparison, whose
# record is written behind its check (samples_differing where the test counts them).
BARS = {
    "wave_lps": [("max_rel_mag_err", WAVE_BAR)],
    "enhance_waves lps": [("wave_err", WAVE_BAR), ("zero_frames_err", WAVE_BAR), ("out_net_relerr", 1e-4)],
    "enhance_waves mask": [("wave_err", WAVE_BAR), ("out_net_relerr", 1e-4)],
    "stream_open": "bits", "stream_open rowinv": "bits", "logmmse_stream_open": "bits", "eval_mix": "bits",
    "mix_features": [("lps_3", 1e-5), ("lps_4", 1e-5), ("irm_3", 1e-4), ("ibm_excluded_share", 1e-3)],
    "score_waves": [("ssnr_db", 1e-4), ("lsd_rel", 1e-3), ("lsd_rel_gpu_lps", 1e-5), ("stoi_abs", 1e-4)],
    "logmmse_waves": [("vad", 1e-4), ("pcm", 1e-4), ("gain_absY", 1e-4)],
}


def cell_figure(entry, fea_dim, record):
    """(text, value, bar) of a cell from the record its test left in the parity JSON (conftest.py), or None without one."""
    if record is None:
        return None
    if BARS[entry] == "bits":
        n = int(record.get("samples_differing", 0))
        return "%d samples differ / 0" % n, n, 0
    rec = dict(record)
    if "ibm_cells" in rec:
        rec["ibm_excluded_share"] = rec["ibm_excluded_cells"] / float(rec["ibm_cells"])
    if entry == "logmmse_waves":                                 # per sentence (or per size, the wide call) a dict of the three
        subs = [v for k, v in rec.items() if isinstance(v, dict) and (k[0].isdigit() or k == "fea_dim_%d" % fea_dim)]
        rec = {k: max(v[k] for v in subs) for k, _ in BARS[entry]} if subs else {}
    have = [(rec[k] / bar, k, rec[k], bar) for k, bar in BARS[entry] if k in rec]
    if not have:
        return None
    _, k, v, bar = max(have)
    return "%s %.1e / %.0e" % (k, v, bar), float(v), bar


def numbers_from_records(tests):
    """{"table": {entry: {fea_dim: text}}, "tests": the cells' records} from the "tests" of a parity JSON."""
    table, kept = {}, {}
    for entry, row in COVERAGE.items():
        table[entry] = {}
        for D, cell in row.items():
            fig = cell_figure(entry, D, tests.get(cell))
            assert fig is not None, "no record of %s in the parity JSON" % cell
            table[entry][str(D)] = fig[0]
            kept[cell] = tests[cell]
    for cell in STREAM_MASK.values():
        kept[cell] = tests[cell]
    return {"table": table, "tests": kept}


def markdown_table(numbers=None):
    """The table "entry point x fea_dim -> test" of DESIGN.md 2; with the tests' records (profiles/geometry_parity_numbers.json)
    the worst error and its bar behind every test."""
    rows = ["| entry point | " + " | ".join(str(D) for D in FEA_DIMS) + " |", "|---|" + "---|" * len(FEA_DIMS)]
    for entry, cells in COVERAGE.items():
        line = []
        for D in FEA_DIMS:
            short = cells[D].split("::")[1]
            fig = (numbers or {}).get(entry, {}).get(str(D))
            line.append("`%s`%s" % (short, "<br>%s" % fig if fig else ""))
        rows.append("| `%s` | %s |" % (entry, " | ".join(line)))
    return "\n".join(rows)


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "geometry_parity_numbers.json")
    if sys.argv[1:2] == ["numbers"]:                             # python tests/geometry_cases.py numbers <parity JSON of a -m gpu run>
        src = json.load(open(sys.argv[2]))
        out = numbers_from_records(src["tests"])
        out["written"] = src.get("written")
        json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print(markdown_table(json.load(open(path)).get("table") if os.path.exists(path) else None))
