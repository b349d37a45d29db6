"""A model of one bp_handle across calls, and the walks that tests/test_sequence_gpu.py runs through it.  Imports neither the
package nor a GPU: tests/test_sequence_coverage.py checks everything in here on any machine.

What a handle carries from one call to the next (two stacked buffer pairs, two window staging sets, the tile that the output layer's
launch pre-stages, the split-K ticket words, the Philox step counter, the bf16 weight shadow, the resident corpus, the grow-only work
buffers, the forward mode, the output switches) is invisible to a caller.  What a caller CAN know is the model state below:

    maker, rows, windows, has_targ   which call made the resident chunk, its rows, its kind, and whether that call supplied targets
    preset                           the hyper-parameter preset (PRESETS)
    out                              the output setting (Config.outs)
    fwd                              the forward mode (0 default, 1 row-invariant)
    bunches                          training bunches so far (= the position of the dropout stream)

KINDS is the one table of call kinds.  Each entry has four fields: `pre` (the precondition in model terms: None when it holds, else
the name of what is wrong), `training` (changes weights or momentum, or a switch that training reads: the replay handle R repeats
it; a query is left out of R), `apply` (how a successful call changes the model state) and `fail` (the status the call returns for
each way its precondition can fail, BP_ERR_ARG or BP_ERR_STATE; the model state stays as it was; empty: no precondition).  The rule for what include/bp_c_api.h left open before this
model was written, now stated there: a training or gradient call on a chunk whose targets were not supplied by the call that made
it resident is BP_ERR_STATE.

Data of every call is a function of (configuration, walk, position in the walk) alone (call_data), so the subject, the replay and
every fresh handle see identical bytes."""
import collections

import numpy as np

import mix_np as MX

BP_OK, BP_ERR_ARG, BP_ERR_STATE = 0, -1, -3
STATUS_NAMES = {BP_OK: "BP_OK", BP_ERR_ARG: "BP_ERR_ARG", BP_ERR_STATE: "BP_ERR_STATE"}

FEA_DIM, CONTEXT, TARG_OFFSET, CAP = 33, 3, 1, 256            # n_fft 64, hop 32; NAT: layersizes[0] = (CONTEXT + 1) * FEA_DIM
HOP = FEA_DIM - 1
# (lrate, momentum, weightcost, dropoutflag): the omit rates stay 0.1 / 0.2
PRESETS = [(0.002, 0.5, 1e-4, 1), (0.001, 0.9, 0.0, 0), (0.004, 0.0, 1e-3, 1)]
VISIBLE_OMIT, HID_OMIT = 0.1, 0.2

Config = collections.namedtuple("Config", "id index ls B act dtype outs corpus_target")
CONFIGS = [
    # logistic on columns 33..65 (cross-entropy, then squared error), then linear
    Config("A", 0, [132, 64, 66], 16, 0, 0, [(1, 33, 0), (1, 33, 1), (0, 0, 0)], "lps+irm"),
    # the smallest net whose output layer is split (bp_out_split_stage: the pre-staged tile, the ticket words); linear output only
    Config("B", 1, [132, 1024, 33], 32, 1, 0, [(0, 0, 0)], "lps"),
    Config("C", 2, [132, 64, 66], 16, 0, 1, [(1, 33, 0), (1, 33, 1), (0, 0, 0)], "lps+irm"),
]
BY_ID = {c.id: c for c in CONFIGS}

# ------------------------------------------------------------------ sizes (the smallest that still have a partial bunch)
CLEAN_LEN = [200, 330, 97, 1000]                              # T = (n - 1) // HOP + 2 = 8, 12, 5, 33 frames
NOISE_LEN = [500, 37, 3000]
SNRS = [-5.0, 0.0, 5.0, 10.0]
QUERY_CLEAN = [0, 3]                                          # CrossValid_mix, mix_features, eval_mix: 41 frames (more than either bunch)
ENHANCE_LEN = [200, 1000]                                     # enhance_waves: 41 frames
STREAM_LEN, STREAM_BLOCKS = 200, [70, 33, 97]                 # 8 frames, all of them due with the last block (the NAT row needs 6)
SAMPLE_RATE = 8000


def frames_of(n_samples):
    return (n_samples - 1) // HOP + 2


def train_rows(cfg):
    return 2 * cfg.B + cfg.B // 2


def query_rows(cfg):
    return cfg.B + 3


def train_clean(cfg):
    """The clean entries of a train_mix call: the fewest of the long sentence (plus one short) that give two bunches and a part."""
    out, T = [], 0
    while T < 2 * cfg.B + 1:
        out.append(3)
        T += frames_of(CLEAN_LEN[3])
    if T % cfg.B == 0:
        out.append(2)
    return out


def mix_rows(clean):
    return int(sum(frames_of(CLEAN_LEN[c]) for c in clean))


# ------------------------------------------------------------------ the model
def fresh_state():
    return dict(maker=None, maker_kind=None, rows=0, windows=False, has_targ=False, preset=0, out=0, fwd=0, bunches=0)


def _resident(st, pos, kind, rows, windows, has_targ):
    st.update(maker=pos, maker_kind=kind, rows=rows, windows=windows, has_targ=has_targ)


def _pre_none(cfg, st):
    return None


def _pre_resident_bunch(cfg, st):
    """train_resident(0, B) and grads_resident(0): one bunch of whatever is resident."""
    if st["rows"] < cfg.B:
        return "range"                                         # frame range outside the resident chunk (checked first)
    if not st["has_targ"]:
        return "no targets"                                    # the call that made the chunk resident supplied no targets
    return None


_FAIL_RESIDENT_BUNCH = {"range": BP_ERR_ARG, "no targets": BP_ERR_STATE}


def _pre_set_forward(cfg, st):
    return "bf16" if cfg.dtype == 1 else None                  # the bf16 forward has no row-invariant kernel


def _ap_train(cfg, st, pos):
    _resident(st, pos, "train", train_rows(cfg), False, True)
    st["bunches"] += train_rows(cfg) // cfg.B


def _ap_train_windows(cfg, st, pos):
    _resident(st, pos, "train_windows", train_rows(cfg), True, True)
    st["bunches"] += train_rows(cfg) // cfg.B


def _ap_upload_train(cfg, st, pos):
    _resident(st, pos, "upload_train", train_rows(cfg), False, True)
    st["bunches"] += 3                                         # train_resident(B, B) and train_resident(0, 2B)


def _ap_train_resident(cfg, st, pos):
    st["bunches"] += 1


def _ap_train_mix(cfg, st, pos):
    T = mix_rows(train_clean(cfg))
    _resident(st, pos, "train_mix", T, True, True)
    st["bunches"] += T // cfg.B


def _ap_preset(cfg, st, pos):
    st["preset"] = (st["preset"] + 1) % len(PRESETS)


def _ap_set_output(cfg, st, pos):
    st["out"] = (st["out"] + 1) % len(cfg.outs)


def _ap_query_chunk(kind, windows, has_targ, rows):
    def ap(cfg, st, pos):
        _resident(st, pos, kind, rows(cfg), windows, has_targ)
    return ap


def _ap_set_forward(cfg, st, pos):
    st["fwd"] ^= 1


def _ap_nothing(cfg, st, pos):
    pass


Kind = collections.namedtuple("Kind", "name pre training apply fail")
_q41 = lambda cfg: mix_rows(QUERY_CLEAN)
KINDS = collections.OrderedDict((k.name, k) for k in [
    Kind("train", _pre_none, True, _ap_train, {}),
    Kind("train_windows", _pre_none, True, _ap_train_windows, {}),
    Kind("upload_train", _pre_none, True, _ap_upload_train, {}),
    Kind("train_resident", _pre_resident_bunch, True, _ap_train_resident, _FAIL_RESIDENT_BUNCH),
    Kind("train_mix", _pre_none, True, _ap_train_mix, {}),
    Kind("preset", _pre_none, True, _ap_preset, {}),
    Kind("set_output", _pre_none, True, _ap_set_output, {}),
    Kind("forward", _pre_none, False, _ap_query_chunk("forward", False, False, query_rows), {}),
    Kind("cv", _pre_none, False, _ap_query_chunk("cv", False, False, query_rows), {}),
    Kind("cv_windows", _pre_none, False, _ap_query_chunk("cv_windows", True, False, query_rows), {}),
    Kind("cv_mix", _pre_none, False, _ap_query_chunk("cv_mix", True, False, _q41), {}),
    # (bp_mix_features makes the targets on the device and leaves them with the chunk: training on it is legal)
    Kind("mix_features", _pre_none, False, _ap_query_chunk("mix_features", True, True, _q41), {}),
    Kind("enhance", _pre_none, False, _ap_query_chunk("enhance", True, False, lambda cfg: sum(frames_of(n) for n in ENHANCE_LEN)), {}),
    Kind("eval_mix", _pre_none, False, _ap_query_chunk("eval_mix", True, False, _q41), {}),
    Kind("grads", _pre_none, False, _ap_query_chunk("grads", False, True, query_rows), {}),
    # the gradient of the first bunch of WHATEVER is resident, stacked or window, legal or refused as train_resident(0, B) is; it
    # leaves the chunk, the weights and the dropout stream where they were
    Kind("grads_resident", _pre_resident_bunch, False, _ap_nothing, _FAIL_RESIDENT_BUNCH),
    # (only the last push has frames due: its 8 rows, fewer than either bunch, become the resident chunk)
    Kind("stream", _pre_none, False, _ap_query_chunk("stream", True, False, lambda cfg: frames_of(STREAM_LEN)), {}),
    Kind("set_forward", _pre_set_forward, False, _ap_set_forward, {"bf16": BP_ERR_ARG}),
    Kind("checkpoint", _pre_none, False, _ap_nothing, {}),
])
# query kinds that make a chunk WITH targets resident: the replay handle, which leaves queries out, loads their chunk when a
# later train_resident trains on it
LOADABLE = ("mix_features", "grads")


def kinds_of(cfg):
    """set_output applies only where the net has logistic columns."""
    return [k for k in KINDS if k != "set_output" or len(cfg.outs) > 1]


Step = collections.namedtuple("Step", "pos kind status before after")


def run_model(cfg, calls, st=None):
    """The model over calls = [(pos, kind), ...] from a fresh handle: one Step per call with the expected status and the model
    state before and after it."""
    st = fresh_state() if st is None else dict(st)
    out = []
    for pos, kind in calls:
        k = KINDS[kind]
        before = dict(st)
        why = k.pre(cfg, st)
        status = BP_OK if why is None else k.fail[why]
        if why is None:
            k.apply(cfg, st, pos)
        out.append(Step(pos, kind, status, before, dict(st)))
    return out


# ------------------------------------------------------------------ the walks
def closed_walk(cfg):
    """Kinds of one closed walk that takes every ordered pair (kind, next kind) exactly once: an Eulerian circuit of the complete
    directed graph with loops on the configuration's kinds (Hierholzer; the order of each node's edges from a seeded shuffle).
    K * K + 1 entries, the last one the first again."""
    ks = kinds_of(cfg)
    K = len(ks)
    rng = np.random.default_rng([cfg.index, 7])
    nxt = [list(rng.permutation(K)) for _ in range(K)]
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(int(nxt[v].pop()))
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == K * K + 1 and circuit[0] == circuit[-1]
    return [ks[i] for i in circuit]


# Pieces of the closed walk, each a GPU test of its own from a fresh subject and replay.  A whole closed walk takes about two
# seconds on an MI355X (362 calls on three handles and some 200 fresh ones), under the ten it may take: ONE piece.  With more, a
# piece starts with the call that the piece before it ended with, so that no pair is dropped at a cut.
N_PIECES = 1
N_RANDOM, RANDOM_LEN = 4, 60


def _piece_id(i, n=None):
    return "closed" if (N_PIECES if n is None else n) == 1 else "closed%d" % i


def pieces(cfg, n_pieces=None):
    """[(pos, kind), ...] per piece; pos is the index in the closed walk (it selects the data)."""
    P = N_PIECES if n_pieces is None else n_pieces
    w = closed_walk(cfg)
    n = len(w) - 1
    cuts = [round(i * n / P) for i in range(P + 1)]
    return [[(p, w[p]) for p in range(cuts[i], cuts[i + 1] + 1)] for i in range(P)]


def random_walk(cfg, seed):
    ks = kinds_of(cfg)
    rng = np.random.default_rng([cfg.index, 1000 + seed])
    return [(p, ks[int(rng.integers(len(ks)))]) for p in range(RANDOM_LEN)]


def walk_ids(cfg):
    return [_piece_id(i) for i in range(N_PIECES)] + ["random%d" % s for s in range(N_RANDOM)]


def walk_calls(cfg, wid):
    """(walk number for the data, calls) of one walk id."""
    if wid.startswith("closed"):
        return 0, pieces(cfg)[int(wid[6:] or 0)]
    s = int(wid[6:])
    return 1 + s, random_walk(cfg, s)


def pair_table(cfg, n_pieces=None):
    """(kind, next kind) -> the pieces that run it."""
    out = {}
    for i, p in enumerate(pieces(cfg, n_pieces)):
        for (_, a), (_, b) in zip(p, p[1:]):
            out.setdefault((a, b), []).append(_piece_id(i, n_pieces))
    return out


def test_id(cfg, wid):
    return "tests/test_sequence_gpu.py::test_walk[%s-%s]" % (cfg.id, wid)


GPU_TESTS = [test_id(c, w) for c in CONFIGS for w in walk_ids(c)]


# ------------------------------------------------------------------ data
def corpus(cfg):
    rng = np.random.default_rng([cfg.index, 99])
    clean = [(rng.normal(size=n) * 3000.0).astype(np.float32) + np.float32(0.0) for n in CLEAN_LEN]
    noise = [(rng.normal(size=n) * 1500.0).astype(np.float32) for n in NOISE_LEN]
    mean = rng.normal(10.0, 2.0, FEA_DIM).astype(np.float32)
    inv_std = rng.uniform(0.2, 0.5, FEA_DIM).astype(np.float32)
    return dict(clean=clean, noise=noise, mean=mean, inv_std=inv_std)


def _targets(cfg, rng, n):
    sL = cfg.ls[-1]
    t = rng.normal(size=(n, sL)).astype(np.float32)
    if len(cfg.outs) > 1:                                      # the logistic columns: targets in [0, 1]
        t[:, FEA_DIM:] = rng.uniform(size=(n, sL - FEA_DIM)).astype(np.float32)
    return t


def _stacked(cfg, rng, n):
    return dict(x=rng.normal(size=(n, cfg.ls[0])).astype(np.float32), t=_targets(cfg, rng, n))


def _windows(cfg, rng, n):
    nf = n + 7
    ws = rng.integers(0, nf - CONTEXT + 1, n).astype(np.int32)
    return dict(fea=rng.normal(size=(nf, FEA_DIM)).astype(np.float32), targ_frames=_targets(cfg, rng, nf), win_start=ws,
                targ_frame=(ws + TARG_OFFSET).astype(np.int32), nat=rng.normal(size=(2, FEA_DIM)).astype(np.float32),
                nat_row=rng.integers(0, 2, n).astype(np.int32))


def _plan(rng, clean):
    """Rows (clean, noise, offset, snr_db) of a mixture plan."""
    out = []
    for c in clean:
        nz = int(rng.integers(len(NOISE_LEN)))
        out.append((int(c), nz, int(rng.integers(NOISE_LEN[nz])), float(SNRS[int(rng.integers(len(SNRS)))])))
    return out


def call_data(cfg, walk, pos, kind):
    """What the call at position pos of walk number `walk` is made with."""
    rng = np.random.default_rng([cfg.index, walk, pos])
    if kind in ("train", "upload_train"):
        return _stacked(cfg, rng, train_rows(cfg))
    if kind in ("forward", "cv", "grads"):
        return _stacked(cfg, rng, query_rows(cfg))
    if kind == "train_windows":
        return _windows(cfg, rng, train_rows(cfg))
    if kind == "cv_windows":
        return _windows(cfg, rng, query_rows(cfg))
    if kind == "train_mix":
        clean = train_clean(cfg)
        return dict(plan=_plan(rng, clean), order=MX.shuffle(1 + pos, 10 * walk + cfg.index, mix_rows(clean)))
    if kind in ("cv_mix", "mix_features", "eval_mix"):
        return dict(plan=_plan(rng, QUERY_CLEAN))
    if kind == "enhance":
        return dict(sentences=[(rng.normal(size=n) * 3000.0).astype(np.float32) for n in ENHANCE_LEN])
    if kind == "stream":
        x = (rng.normal(size=STREAM_LEN) * 3000.0).astype(np.float32)
        return dict(blocks=np.split(x, np.cumsum(STREAM_BLOCKS)[:-1]))
    return {}


# ------------------------------------------------------------------ the figures of a GPU run
def numbers(parity):
    """The entries of a session's parity JSON (conftest.py) that the walks and the data-parallel life wrote."""
    keep = {k: v for k, v in sorted(parity["tests"].items()) if "test_sequence_gpu.py" in k or "test_dp_life_gpu.py" in k}
    return {"source": "a -m gpu run of tests/test_sequence_gpu.py and tests/test_dp_life_gpu.py on an MI355X; "
                      "`python tests/sequence_model.py numbers <parity JSON> <out>` behind it",
            "bar": "bit for bit: words_differing == 0 in every entry (the life against one rank: 1e-5)", "tests": keep}


if __name__ == "__main__":
    import json
    import sys
    if len(sys.argv) == 4 and sys.argv[1] == "numbers":
        json.dump(numbers(json.load(open(sys.argv[2]))), open(sys.argv[3], "w"), indent=1, sort_keys=True)
    else:
        for cfg in CONFIGS:
            print(cfg.id, " ".join(closed_walk(cfg)))
