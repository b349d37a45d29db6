"""The walks of the four families, pinned: tests/golden/walk_digests.json holds one sha256 per GPU test id of tests/test_sequence_gpu.py,
tests/test_size_gpu.py and tests/test_xsize_gpu.py (260) and one per (family, configuration) corpus (14), recorded from the four separate
models before they became one engine.  A digest covers the walk number, every step of the model run (pos, kind, size where the family
has one, status, the model state before and after) and every call's data, in a canonical form:

    dict        its length, then key and value in sorted key order
    list/tuple  its length, then the items            (a namedtuple: as the dict of its fields)
    ndarray     dtype, shape and the C-contiguous bytes (a numpy scalar: as the 0-d array)
    the rest    the type's name and repr()

`digests(adapter)` takes a family as six functions -- ids, walk_calls, run_model, call_data, corpus, test_id -- over its configurations,
so the same code reads any older layout of the models through a few adapter lines."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_digests.json")
FAMILIES = ("walk", "extended", "size", "xsize")
Adapter = collections.namedtuple("Adapter", "configs sized ids walk_calls run_model call_data corpus test_id")


def feed(h, v):
    if isinstance(v, tuple) and hasattr(v, "_asdict"):
        v = dict(v._asdict())
    if isinstance(v, dict):
        h.update(b"D%d;" % len(v))
        for k in sorted(v):
            feed(h, k)
            feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"L%d;" % len(v))
        for x in v:
            feed(h, x)
    elif isinstance(v, (np.ndarray, np.generic)):
        a = np.ascontiguousarray(v)
        h.update(("A%s%r;" % (a.dtype.str, tuple(np.shape(v)))).encode())
        h.update(a.tobytes())
    else:
        h.update(("%s:%r;" % (type(v).__name__, v)).encode())


def digest(v):
    h = hashlib.sha256()
    feed(h, v)
    return h.hexdigest()


def digests(a):
    """{"tests": {GPU test id: sha256}, "corpus": {configuration id: sha256}} of one family."""
    tests, cor = collections.OrderedDict(), collections.OrderedDict()
    for cfg in a.configs:
        cor[cfg.id] = digest(a.corpus(cfg))
        for wid in a.ids(cfg):
            walk, calls = a.walk_calls(cfg, wid)
            steps = a.run_model(cfg, calls)
            rows = []
            for s in steps:
                row = dict(pos=s.pos, kind=s.kind, status=s.status, before=s.before, after=s.after)
                if a.sized:
                    row["size"] = s.size
                rows.append(row)
            tests[a.test_id(cfg, wid)] = digest(dict(walk=walk, steps=rows, data=[a.call_data(cfg, walk, s) for s in steps]))
    return {"tests": tests, "corpus": cor}


def adapter(name):
    import sequence_model as SM
    import size_model as ZM
    f = ZM.FAMILIES[name]
    return Adapter(f.configs, bool(f.sizes), lambda c: SM.walk_ids(f, c), lambda c, w: SM.walk_calls(f, c, w), lambda c, calls: SM.run_model(f, c, calls),
                   lambda c, walk, s: SM.call_data(f, c, walk, s.pos, s.kind, s.size), lambda c: SM.corpus(f, c), lambda c, w: SM.test_id(f, c, w))


@pytest.mark.parametrize("family", FAMILIES)
def test_every_walk_is_the_walk_that_was_recorded(family):
    want = json.load(open(GOLDEN))[family]
    got = digests(adapter(family))
    assert sorted(got["tests"]) == sorted(want["tests"]), (sorted(set(want["tests"]) - set(got["tests"])), sorted(set(got["tests"]) - set(want["tests"])))
    assert sorted(got["corpus"]) == sorted(want["corpus"])
    differ = [k for part in ("corpus", "tests") for k in want[part] if got[part][k] != want[part][k]]
    assert differ == [], differ


def test_the_record_holds_260_tests_and_14_corpora():
    rec = json.load(open(GOLDEN))
    assert sorted(rec) == sorted(FAMILIES)
    assert [len(rec[f]["tests"]) for f in FAMILIES] == [15, 24, 69, 152] and [len(rec[f]["corpus"]) for f in FAMILIES] == [3, 4, 3, 4]
    assert len(set(t for f in FAMILIES for t in rec[f]["tests"])) == 260
