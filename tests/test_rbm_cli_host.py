"""bppretrain up to the point where it would use the device (no GPU): exit status, every byte of stdout and of
the log file for command lines that all end before any device call -- the refusals of its keys and values, in the tools'
convention (a message, exit status 0).  Fixtures and the <TMP> / <LOG> convention are those of tests/test_cli_host.py; the expected
texts are in tests/golden/rbm_cli_messages.json:

    python tests/test_rbm_cli_host.py record <directory of the binary>

rewrites the file from whatever binary it is given."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cli_host as CH  # noqa: E402

GOLDEN = os.path.join(CH.ROOT, "tests", "golden", "rbm_cli_messages.json")
TOOL = "bppretrain"


def cases():
    p = lambda n: CH.T + "/" + n
    net = ["fea_file=" + p("f.pfile"), "norm_file=" + p("norm5"), "fea_dim=5", "fea_context=3", "targ_offset=1", "layersizes=15,8,6,5",
           "bunchsize=4", "traincache=100", "train_sent_range=0-1", "outwts_file=" + p("pre.wts"), "log_file=<LOG>"]
    swap = lambda key, arg: [arg if a.startswith(key + "=") else a for a in net]
    return [
        ("no_equals", ["fea_dim=5", "rbm_epochs"]), ("unknown_key_ignored", ["bogus=1"]), ("unknown_rbm_key", ["rbm_lrat=0.1"]),
        ("epochs_text", ["rbm_epochs=2x"]), ("epochs_negative", ["rbm_epochs=-1"]), ("epochs_empty_field", ["rbm_epochs=1,,2"]),
        ("epochs_ten_fields", ["rbm_epochs=1,1,1,1,1,1,1,1,1,1,1"]), ("sample_two", ["rbm_sample=2"]), ("sample_text", ["rbm_sample=yes"]),
        ("lrate_text", ["rbm_lrate=fast"]), ("lrate_nan", ["rbm_lrate=nan"]), ("momentum_trailing", ["rbm_momentum=0.5,"]),
        ("weightcost_huge", ["rbm_weightcost=1e400"]), ("first_bad_wins", ["rbm_sample=2", "rbm_lrate=fast"]),
        ("sizes_two", swap("layersizes", "layersizes=15,5")), ("sizes_zero", swap("layersizes", "layersizes=15,0,5")),
        ("bunch_zero", swap("bunchsize", "bunchsize=0")), ("traincache_below_bunch", swap("traincache", "traincache=3")),
        ("device_negative", net + ["device=-1"]),
        ("lrate_negative", net + ["rbm_lrate=-0.1"]), ("momentum_one", net + ["rbm_momentum=0.5,1"]), ("weightcost_negative", net + ["rbm_weightcost=-1e-5"]),
        ("three_values_for_two_layers", net + ["rbm_lrate=0.1,0.2,0.3"]), ("three_epochs_for_two_layers", net + ["rbm_epochs=1,2,3"]),
        ("log_unwritable", swap("log_file", "log_file=" + p("nodir/x.log"))), ("outwts_unwritable", swap("outwts_file", "outwts_file=" + p("nodir/x.wts"))),
        ("fea_missing", swap("fea_file", "fea_file=" + p("nope.pfile"))), ("norm_short", swap("norm_file", "norm_file=" + p("norm5_short"))),
        ("range_format", swap("train_sent_range", "train_sent_range=01") + ["rbm_epochs=1,2", "rbm_sample=0"]),
        ("initwts_missing", net + ["initwts_file=" + p("none.wts"), "rbm_epochs=1", "rbm_lrate=0.002,0.05", "rbm_momentum=0.5", "rbm_weightcost=0", "rbm_sample=1,0"]),
    ]


NAMES = [n for n, _ in cases()]


def run_case(bindir, name, args, d):
    log = os.path.join(d, "%s.%s.log" % (TOOL, name))
    argv = [a.replace("<LOG>", log).replace(CH.T, d) for a in args]
    r = subprocess.run([os.path.join(bindir, TOOL)] + argv, capture_output=True, timeout=60, cwd=d)
    scrub = lambda b: b.decode("utf-8", "replace").replace(log, "<LOG>").replace(d, CH.T)
    got = {"rc": r.returncode, "stdout": scrub(r.stdout), "log": None}
    if os.path.exists(log):
        with open(log, "rb") as f:
            got["log"] = scrub(f.read())
    assert r.stderr == b"", r.stderr
    return got


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rbm_cli"))
    CH.make_fixtures(d)
    return d


@pytest.fixture(scope="module")
def bindir():
    if not os.path.exists(os.path.join(CH.PKG, TOOL)):
        import __graft_entry__
        __graft_entry__.build()
    return CH.PKG


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_record(golden):
    assert sorted(NAMES) == sorted(golden) and len(set(NAMES)) == len(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_messages_are_those_of_the_record(bindir, fixtures, golden, name):
    args = dict(cases())[name]
    got = run_case(bindir, name, args, fixtures)
    assert got == golden[name], args
    assert got["rc"] == 0 and "all finish!" not in got["stdout"]
    assert got["stdout"] or got["log"]                      # every refusal says why, on stdout or in the log


def test_the_refusals_name_the_key(golden):
    for name, needle in (("unknown_rbm_key", "unknown key rbm_lrat"), ("epochs_text", "bad value for rbm_epochs: 2x"), ("sample_two", "bad value for rbm_sample: 2"),
                         ("lrate_nan", "bad value for rbm_lrate: nan"), ("first_bad_wins", "rbm_sample"), ("lrate_negative", "rbm_lrate must be >= 0"),
                         ("momentum_one", "rbm_momentum must lie in [0, 1)"), ("three_values_for_two_layers", "one value or one per hidden layer (2)"),
                         ("sizes_two", "need 3..9 layer sizes"), ("no_equals", "Format Error")):
        assert needle in golden[name]["stdout"], name
    assert "can not open initial weights file" in golden["initwts_missing"]["log"]


def record(bindir):
    with tempfile.TemporaryDirectory(prefix="rbm_cli_record_") as d:
        CH.make_fixtures(d)
        out = {name: run_case(bindir, name, args, d) for name, args in cases()}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "record", __doc__
    record(os.path.abspath(sys.argv[2]))
