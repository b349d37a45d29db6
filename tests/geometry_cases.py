"""The frame sizes of the signal layer and, for every public entry point that takes a fea_dim, the GPU test that holds it to a
reference at each of them (tests/test_geometry_coverage.py checks without a GPU that every cell names a test that exists;
tests/test_geometry_gpu.py holds the cases that no older file had the body for).

What changes with the size (csrc/bp_fft.h): the trip counts of fft_lds / rfft_frame / synth_frame (less than one item per thread
at 33, five bins per thread at 1025), the padded LDS index and the dynamic LDS sizes, and the workgroups per sentence of the two
noise-aware-row kernels (kb = ceil(D / 256): one up to 129, two at 257, three at 513, five at 1025).  For the entry points added
since: NB, the bins per thread of bp_lmstream_push<NB, SPP> and of the PostFn synthesis kernels (1 up to 129, 2 at 257, 3 at 513,
5 at 1025), whose per-channel lam / Ap / pb state is indexed by the clamped bin; ceil(D / 64), the 64-thread workgroups per
sentence or job of bp_wave_dnat and bp_stream_dnat and the column blocks of bp_wave_gv_parts (1, 2 -- the second with one live
thread -- 3, 5, 9, 17); the dynamic LDS of bp_wave_mel (the FFT, then P[M + 1], then the filters' words: other offsets and trip
counts at every size); and the LDS of bp_stream_synthesis<PostFn> (the FFT space and S, then two frames of 2 M floats: the large
layout from 257 on).

A cell is "tests/<file>.py::<test>[<id>]", the id as pytest prints it.  The stream cells compare bit for bit with the offline call
of the same size, which the `enhance_waves` rows hold to the float64 restatement; eval_mix compares bit for bit with its parts.

API (below) maps every bp_* symbol of include/bp_c_api.h to the rows that hold it, or to the reason it has no frame size;
tests/test_geometry_coverage.py fails on a symbol that is not classified, so an entry point added later cannot stay outside."""
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


def _mel_ids():
    """{fea_dim: the id of mel_np's geometry at that size}: one geometry per size."""
    import mel_np
    out = {g["fea_dim"]: mel_np.geo_id(g) for g in mel_np.GEOMETRIES}
    assert len(out) == len(mel_np.GEOMETRIES), "mel_np.GEOMETRIES: two geometries of one fea_dim"
    return out


GEO = "tests/test_geometry_gpu.py::"
NOISE, DNAT, POST = "tests/test_noise_gpu.py::", "tests/test_dnat_gpu.py::", "tests/test_post_gpu.py::"
MEL_IDS = _mel_ids()
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
    # ---- the entry points added after the table was first closed
    "logmmse_waves spp": _merge(_per_size(NOISE + "test_tracker_matches_restatement[%d]", [33, 65, 129, 257]),
                                {D: NOISE + "test_tracker_wide_spectrum_paths" for D in (513, 1025)}),
    "logmmse_stream_open spp": _per_size(NOISE + "test_tracker_streams_return_the_offline_bits[%d]"),
    "enhance_waves dynamic": _merge(_per_size(DNAT + "test_rows_match_restatement_and_the_baseline[%d-3-1]", [33, 65, 129, 513, 1025]),
                                    {257: DNAT + "test_rows_match_restatement_and_the_baseline[257-1-0]"}),
    "mix_features dynamic": _merge(_per_size(DNAT + "test_rows_match_restatement_and_the_baseline[%d-3-1]", [33, 65, 129, 513, 1025]),
                                   {257: DNAT + "test_rows_match_restatement_and_the_baseline[257-1-0]"}),
    "stream_open dynamic": _merge(_per_size(DNAT + "test_streams_return_the_bits_of_enhance_waves[%d-3-1-False]", [33, 65, 257, 513, 1025]),
                                  {129: DNAT + "test_streams_return_the_bits_of_enhance_waves[129-1-0-False]"}),
    "train_mix dynamic": _per_size(DNAT + "test_training_equals_host_stacked_rows[%d]"),
    "wave_mfcc": {D: "tests/test_mel_gpu.py::test_wave_mfcc_matches_restatement[%s]" % i for D, i in MEL_IDS.items()},
    "post_rows": _per_size(POST + "test_post_rows_equal_the_restatement[both-%d]"),
    "gv_mix raw": _per_size(POST + "test_gv_mix_raw_equals_the_restated_sums[%d]"),
    "gv_mix post": _per_size(POST + "test_gv_mix_post_equals_the_restated_sums[%d-static-False]"),
    "enhance_waves post": _per_size(POST + "test_resynthesis_from_the_post_processed_rows[%d]"),
    "stream_open post": _per_size(POST + "test_paths_agree_bit_for_bit[%d]"),
}
# the mask target at an odd column offset of a padded output row (out_col = D), streamed
STREAM_MASK = _per_size("tests/test_stream_gpu.py::test_other_configurations[fea%d_mask]", [257, 1025])
# Cells beside the table: a path that one size is enough for, because the kernel behind it is held at every size by a row above.
EXTRA = {
    "stream_open mask": STREAM_MASK,
    # the packed (row-invariant) stream in dynamic mode, at the smallest and the largest size
    "stream_open dynamic rowinv": _per_size(DNAT + "test_streams_return_the_bits_of_enhance_waves[%d-3-1-True]", [33, 1025]),
    # bp_set_mix_aux: the MFCC columns of a mixing call behind a wide LPS block (two bins per thread)
    "set_mix_aux": {257: "tests/test_mel_gpu.py::test_mfcc_columns_are_wave_mfcc_of_the_target_signal[lps+irm-257]"},
}


# Every bp_* symbol of include/bp_c_api.h: the COVERAGE rows that hold it at the six sizes (a tuple), or the reason it has no frame
# size (a string).  A symbol whose prototype takes a fea_dim has rows, or a reason that begins with "host only".
_HOST = "host only"
_STEP = "the net's step: rows of any width, no fea_dim"
_SAMPLES = "no fea_dim: sample-domain"
_DP = "the data-parallel exchange: no fea_dim"
_RBM = "pre-training: rows of any width, no fea_dim"
_NET_STREAMS = ("stream_open", "stream_open rowinv", "stream_open dynamic", "stream_open post")
_LM_STREAMS = ("logmmse_stream_open", "logmmse_stream_open spp")
_MIX = ("mix_features", "mix_features dynamic")
API = {
    "bp_last_error": _HOST, "bp_abi_version": _HOST, "bp_build_target": _HOST, "bp_device_count": _HOST,
    "bp_create": _STEP, "bp_destroy": _STEP, "bp_set_hyper": _STEP, "bp_set_output": _STEP, "bp_set_forward": _STEP,
    "bp_train_chunk": _STEP, "bp_cv_chunk": _STEP, "bp_forward": _STEP, "bp_get_weights": _STEP, "bp_get_deltas": _STEP,
    "bp_upload_chunk": _STEP, "bp_fill_chunk_synthetic": _STEP, "bp_train_resident": _STEP, "bp_sync": _STEP,
    "bp_train_resident_masked": _STEP, "bp_upload_chunk_windows": _STEP, "bp_train_chunk_windows": _STEP,
    "bp_cv_chunk_windows": _STEP, "bp_forward_windows": _STEP,
    "bp_enhance_waves": ("enhance_waves lps", "enhance_waves mask", "enhance_waves dynamic", "enhance_waves post"),
    "bp_wave_lps": ("wave_lps",),
    # the mixing calls stage their rows with the kernels of bp_mix_features, then run the net's step
    "bp_set_mix_corpus": _MIX, "bp_mix_features": _MIX, "bp_cv_mix": _MIX, "bp_train_mix": _MIX + ("train_mix dynamic",),
    "bp_mix_plan": _HOST, "bp_mix_shuffle": _HOST,
    "bp_mel_defaults": _HOST, "bp_mel_dct": _HOST,
    "bp_mel_filters": _HOST + ": the filter table (tests/test_mel_host.py holds it at one geometry per size)",
    "bp_wave_mfcc": ("wave_mfcc",), "bp_set_mix_aux": ("wave_mfcc",),
    "bp_set_mix_reverb": _SAMPLES, "bp_reverb_waves": _SAMPLES, "bp_mix_rir_delay": _HOST, "bp_mix_reverb_pairs": _HOST,
    "bp_rir_image": _SAMPLES, "bp_rir_orders": _HOST, "bp_rir_beta": _HOST, "bp_rir_rooms": _HOST,
    "bp_score_waves": ("score_waves",), "bp_score_waves_ext": ("score_waves",),
    "bp_eval_mix": ("eval_mix",), "bp_eval_mix_ext": ("eval_mix",),
    "bp_logmmse_defaults": _HOST, "bp_noise_defaults": _HOST,
    "bp_logmmse_waves": ("logmmse_waves",), "bp_logmmse_waves_nt": ("logmmse_waves", "logmmse_waves spp"),
    # bit for bit their parts (tests/test_classic_gpu.py, tests/test_noise_gpu.py): the mixture, the baseline, the scores
    "bp_eval_mix_logmmse": ("mix_features", "logmmse_waves", "score_waves"),
    "bp_eval_mix_logmmse_ext": ("mix_features", "logmmse_waves", "score_waves"),
    "bp_eval_mix_logmmse_nt": ("mix_features", "logmmse_waves", "logmmse_waves spp", "score_waves"),
    "bp_stream_open": _NET_STREAMS, "bp_stream_push": _NET_STREAMS, "bp_stream_close": _NET_STREAMS, "bp_stream_packed": _HOST,
    "bp_stream_counts": _HOST + ": frame counts (test_the_library_accepts_exactly_the_six_sizes probes every size)",
    "bp_lmstream_open": ("logmmse_stream_open",), "bp_lmstream_open_nt": _LM_STREAMS, "bp_lmstream_push": _LM_STREAMS,
    "bp_lmstream_close": _LM_STREAMS,
    "bp_lmstream_counts": _HOST + ": frame counts (test_the_library_accepts_exactly_the_six_sizes probes every size)",
    "bp_set_nat": ("enhance_waves dynamic", "mix_features dynamic", "stream_open dynamic", "train_mix dynamic"),
    "bp_post_defaults": _HOST, "bp_set_post": ("enhance_waves post", "stream_open post", "gv_mix post"),
    "bp_post_rows": ("post_rows",), "bp_gv_mix": ("gv_mix raw", "gv_mix post"),
    "bp_gv_factors": _HOST + ": fea_dim is the length of the four sums (tests/test_post_host.py)",
    "bp_resample_defaults": _HOST, "bp_resample_ratio": _HOST, "bp_resample_len": _HOST, "bp_resample_taps": _HOST,
    "bp_resample_waves": _SAMPLES,
    "bp_grads_resident": _STEP, "bp_grad_floats": _STEP, "bp_grad_layout": _STEP, "bp_read_grads": _STEP, "bp_read_layer_output": _STEP,
    "bp_dp_attach": _DP, "bp_dp_attach_ex": _DP, "bp_dp_detach": _DP, "bp_dp_info": _DP, "bp_dp_peer_info": _DP, "bp_dp_handoff": _DP,
    "bp_dp_barrier": _DP, "bp_dp_allgather": _DP, "bp_rdv_open": _HOST, "bp_rdv_barrier": _HOST, "bp_rdv_allgather": _HOST,
    "bp_rdv_close": _HOST, "bp_host_register": _HOST, "bp_host_unregister": _HOST, "bp_device_pci_bus_id": _HOST,
    "bp_last_train_ms": _STEP, "bp_time_kernel": _STEP, "bp_profile_step": _STEP, "bp_measure_peaks": _STEP,
    "bp_rbm_defaults": _HOST, "bp_rbm_create": _RBM, "bp_rbm_destroy": _RBM, "bp_rbm_set_hyper": _RBM, "bp_rbm_train_chunk": _RBM,
    "bp_rbm_up": _RBM, "bp_rbm_step": _RBM, "bp_rbm_steps": _RBM, "bp_rbm_get": _RBM,
}


_PROTOTYPE = r"^([A-Za-z_][A-Za-z0-9_ ]*[ *])(bp_[a-z0-9_]+)\(([^;]*)\);"


def api_prototypes(header_text):
    """{symbol: parameter text} of the bp_* prototypes of a C header: declarations that start a line (comments do not)."""
    import re
    return {m.group(2): m.group(3) for m in re.finditer(_PROTOTYPE, header_text, re.M)}


def api_return_types(header_text):
    """{symbol: return type text} of the same prototypes."""
    import re
    return {m.group(2): " ".join(m.group(1).split()) for m in re.finditer(_PROTOTYPE, header_text, re.M)}


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
            axes.append([str(given(v) if callable(given) else given[k]) if given else _value_id(v) for k, v in enumerate(m.args[1])])
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
    "logmmse_waves spp": [("vad", 1e-4), ("pcm", 1e-4), ("gain_absY", 1e-4), ("noise", 1e-4)],
    "enhance_waves dynamic": [("rows", 1e-4), ("net", 1e-4), ("busy_rows", 1e-4), ("busy_net", 1e-4)],
    "mix_features dynamic": [("rows", 1e-4), ("baseline", 1e-4), ("busy_rows", 1e-4), ("busy_baseline", 1e-4)],
    "wave_mfcc": [("sqrt_power_rel", WAVE_BAR), ("logmel_ulp", 5.0)],     # (the cepstrum: np.array_equal inside the test)
    "enhance_waves post": [("wave_err", WAVE_BAR)],
    "logmmse_stream_open spp": "bits", "stream_open dynamic": "bits", "stream_open post": "bits",
    # "words": word for word with the restatement or the host-stacked run; the record counts the differing words, green is 0
    "train_mix dynamic": "words", "post_rows": "words", "gv_mix raw": "words", "gv_mix post": "words",
}


def cell_figure(entry, fea_dim, record):
    """(text, value, bar) of a cell from the record its test left in the parity JSON (conftest.py), or None without one."""
    if record is None:
        return None
    if BARS[entry] == "bits":
        n = int(record.get("samples_differing", 0))
        return "%d samples differ / 0" % n, n, 0
    if BARS[entry] == "words":
        have = [v for k, v in record.items() if k.startswith("words_differing")]
        if not have:
            return None
        n = sum(sum(int(x) for x in v.values()) if isinstance(v, dict) else int(v) for v in have)
        return "%d words differ / 0" % n, n, 0
    rec = dict(record)
    if "ibm_cells" in rec:
        rec["ibm_excluded_share"] = rec["ibm_excluded_cells"] / float(rec["ibm_cells"])
    if entry in ("logmmse_waves", "logmmse_waves spp"):          # per sentence (or per size, the wide call) a dict of the three
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
    for row in EXTRA.values():
        for cell in row.values():
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
