"""The post-processing keys of bpeval and bpenhance up to the point where the tools would use the device (no
GPU): exit status and every byte of stdout for command lines that all end before any device call.  The fixtures, the runner and the
<TMP> convention are those of tests/test_cli_host.py; the expected texts are in tests/golden/post_cli_messages.json:

    python tests/test_post_cli_host.py record <directory of the binaries>

rewrites the file from whatever binaries it is given."""
import json
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cli_host as CH  # noqa: E402

GOLDEN = os.path.join(CH.ROOT, "tests", "golden", "post_cli_messages.json")


def cases():
    p = lambda n: CH.T + "/" + n
    net = ["fea_context=3", "layersizes=99,64,66", "bunchsize=32", "traincache=2000"]
    ev = ["fea_dim=33", "clean_list=" + p("clean.list"), "noise_list=" + p("noise.list")] + net + ["norm_file=" + p("norm33"), "initwts_file=" + p("none.wts")]
    enh = ["fea_dim=33", "fea_context=3", "layersizes=99,64,66", "norm_file=" + p("norm33"), "initwts_file=" + p("none.wts"),
           "in_wav=" + p("a.wav"), "out_wav=" + p("out_a.wav")]
    c = {}
    c["bpeval"] = [
        ("mask_col_neg", ["post_mask_col=-1"]), ("mask_col_text", ["post_mask_col=3x"]), ("weight_high", ["post_mask_weight=1.5"]),
        ("weight_neg", ["post_mask_weight=-0.1"]), ("lo_nan", ["post_mask_lo=nan"]), ("hi_text", ["post_mask_hi=high"]), ("gv_mode_name", ["gv_mode=both"]),
        ("gv_mode_alone", ev + ["gv_mode=dep"]), ("gate_without_col", ev + ["post_mask_lo=0.3"]),
        ("lo_above_hi", ev + ["post_mask_col=33", "post_mask_lo=0.8", "post_mask_hi=0.2"]),
        ("post_with_mask_target", ev + ["post_gv=" + p("norm33"), "wave_target=mask"]),
        ("gv_out_with_post", ev + ["gv_out=" + p("gv.norm"), "post_gv=" + p("norm33")]),
        ("gv_out_with_baseline", ev + ["gv_out=" + p("gv.norm"), "baseline=logmmse"]),
        ("gv_out_with_scores_out", ev + ["gv_out=" + p("gv.norm"), "scores_out=" + p("s.txt")]),
        ("gv_out_with_mask_target", ev + ["gv_out=" + p("gv.norm"), "wave_target=mask", "out_col=33"]),
        ("pairs_post_key", ["fea_dim=33", "pairs_list=" + p("pairs.list"), "post_mask_col=0"]),
        ("post_then_initwts_missing", ev + ["post_gv=" + p("norm33"), "post_mask_col=33", "post_mask_lo=0.3", "post_mask_hi=0.7", "post_mask_weight=0.5"]),
        ("gv_out_then_initwts_missing", ev + ["gv_out=" + p("gv.norm"), "gv_mode=dep"]),
    ]
    c["bpenhance"] = [
        ("mask_col_neg", ["post_mask_col=-1"]), ("mask_col_text", ["post_mask_col=3x"]), ("weight_high", ["post_mask_weight=1.5"]),
        ("lo_text", ["post_mask_lo=abc"]), ("hi_inf", ["post_mask_hi=inf"]),
        ("gate_without_col", enh + ["post_mask_weight=0.5"]), ("lo_above_hi", enh + ["post_mask_col=33", "post_mask_lo=0.8", "post_mask_hi=0.2"]),
        ("post_with_mask_target", enh + ["post_mask_col=33", "wave_target=mask"]), ("mask_col_high", enh + ["post_mask_col=34"]),
        ("logmmse_post_key", ["method=logmmse", "fea_dim=33", "post_gv=" + p("norm33"), "in_wav=" + p("a.wav"), "out_wav=" + p("o.wav")]),
        ("post_then_initwts_missing", enh + ["post_gv=" + p("norm33"), "post_mask_col=33"]),
    ]
    return c


ALL = [(tool, name) for tool, cs in cases().items() for name, _ in cs]


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("post_cli"))
    CH.make_fixtures(d)
    return d


@pytest.fixture(scope="module")
def bindir():
    if not all(os.path.exists(os.path.join(CH.PKG, t)) for t in cases()):
        import __graft_entry__
        __graft_entry__.build()
    return CH.PKG


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_record(golden):
    assert sorted("%s::%s" % k for k in ALL) == sorted("%s::%s" % (t, n) for t in golden for n in golden[t])


@pytest.mark.parametrize("tool,name", ALL, ids=["%s-%s" % k for k in ALL])
def test_messages_are_those_of_the_record(bindir, fixtures, golden, tool, name):
    args = dict(cases()[tool])[name]
    got = CH.run_case(bindir, tool, name, args, fixtures)
    assert got == golden[tool][name], (tool, args)


def record(bindir):
    out = {}
    with tempfile.TemporaryDirectory(prefix="post_cli_record_") as d:
        CH.make_fixtures(d)
        for tool, cs in cases().items():
            out[tool] = {name: CH.run_case(bindir, tool, name, args, d) for name, args in cs}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "record", __doc__
    record(sys.argv[2])
