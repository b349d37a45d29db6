"""A model of one bp_handle across calls, and the one engine of the walks that tests/test_sequence_gpu.py, tests/test_size_gpu.py and
tests/test_xsize_gpu.py run through it.  Imports neither the package nor a GPU: tests/test_sequence_coverage.py checks everything in
here on any machine, and tests/test_walk_digests.py pins every walk's calls and bytes.

What a handle carries from one call to the next (two stacked buffer pairs, two window staging sets, the tile that the output layer's
launch pre-stages, the split-K ticket words, the Philox step counter, the bf16 weight shadow, the resident corpus, the grow-only work
buffers, the forward mode, the output switches) is invisible to a caller.  What a caller CAN know is the model state below:

    maker, rows, windows, has_targ   which call made the resident chunk, its rows, its kind, and whether that call supplied targets
    preset                           the hyper-parameter preset (PRESETS)
    out                              the output setting (Config.outs)
    fwd                              the forward mode (0 default, 1 row-invariant)
    bunches                          training bunches so far (= the position of the dropout stream)
    nat, maker_nat, post             the noise-aware mode, the mode the resident chunk was made in, and the post-processing setting

KINDS is the one table of call kinds, and API classifies every handle function of the header by the kinds that call it.  Each entry
has four fields: `pre` (the precondition in model terms, of (configuration, state, position): None when it holds, else the name of what
is wrong), `training` (changes weights or momentum, or a switch that training reads: the replay handle R repeats it; a query is left
out of R), `apply` (how a successful call changes the model state) and `fail` (the status the call returns for each way its
precondition can fail, BP_ERR_ARG or BP_ERR_STATE; the model state stays as it was; empty: no precondition).  The rule for what
include/bp_c_api.h left open before this model was written, now stated there: a training or gradient call on a chunk whose targets
were not supplied by the call that made it resident is BP_ERR_STATE.

A Family is a set of walks over the table, as data: WALK (the 19 kinds the table was closed at once, configurations A-C: `test_walk`) and
EXTENDED (all 25, configuration D added: `test_extended_walk`) here, SIZE and XSIZE, which give the calls of those two a size, in
tests/size_model.py.  What the four differ in stands in their records; run_model, the walks, call_data and corpus are one function
each and take the family.

Data of every call is a function of (family, configuration, walk, position in the walk) alone (call_data), so the subject, the replay
and every fresh handle see identical bytes.

Adding a call kind:
  1. one row of KINDS (its precondition, whether the replay repeats it, what it leaves resident, its refusals);
  2. one branch of walk_harness.execute (and of walk_harness.load, if it leaves a chunk with targets: LOADABLE);
  3. its header function(s) in API -- tests/test_sequence_coverage.py fails by name until they are there;
  4. if calls of it come in sizes: its sizes in size_model.SIZES_OF, its shape in size_model.shape and an ask in every row of
     size_model.BUFFERS whose call site it reaches;
  5. the families it joins: EXTENDED and XSIZE take every kind of the table (their closed and random walks then change, and so do
     their records under tests/golden/ and profiles/); WALK and SIZE are closed, NEW_KINDS keeps a new kind out of them."""
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

SAMPLE_RATE, N_CEPS = 8000, 5
AUX = dict(sample_rate=SAMPLE_RATE, n_mel=8, n_ceps=N_CEPS, first_coef=1, lifter=0.0)
RIR_TAPS = [40, 24]
REVERB_PAIRS = [(3, 0), (0, 1)]                                # (clean sentence, response): corpus entries 4 and 5, as long as 3 and 0
REVERB_TARGET, EARLY_TAPS = "early", 10

Config = collections.namedtuple("Config", "id index ls B act dtype outs corpus_target")
CONFIGS = [
    # logistic on columns 33..65 (cross-entropy, then squared error), then linear
    Config("A", 0, [132, 64, 66], 16, 0, 0, [(1, 33, 0), (1, 33, 1), (0, 0, 0)], "lps+irm"),
    # the smallest net whose output layer is split (bp_out_split_stage: the pre-staged tile, the ticket words); linear output only
    Config("B", 1, [132, 1024, 33], 32, 1, 0, [(0, 0, 0)], "lps"),
    Config("C", 2, [132, 64, 66], 16, 0, 1, [(1, 33, 0), (1, 33, 1), (0, 0, 0)], "lps+irm"),
    # fp32, FOUR layers (bp_time_kernel's ids 0..2 need a hidden -> hidden layer), logistic on the mask columns of an output
    # [LPS | MFCC | mask] (bp_set_mix_aux before the corpus), a corpus with bp_set_mix_reverb derived entries that the plans of
    # train_mix / cv_mix / mix_features / eval_mix / gv_mix draw on
    Config("D", 3, [132, 64, 64, 2 * FEA_DIM + N_CEPS], 16, 0, 0, [(1, FEA_DIM + N_CEPS, 0), (1, FEA_DIM + N_CEPS, 1), (0, 0, 0)], "lps+irm"),
]
BY_ID = {c.id: c for c in CONFIGS}

# ------------------------------------------------------------------ sizes (the smallest that still have a partial bunch)
CLEAN_LEN = [200, 330, 97, 1000]                              # T = (n - 1) // HOP + 2 = 8, 12, 5, 33 frames
NOISE_LEN = [500, 37, 3000]
SNRS = [-5.0, 0.0, 5.0, 10.0]
QUERY_CLEAN = [0, 3]                                          # CrossValid_mix, mix_features, eval_mix: 41 frames (more than either bunch)
ENHANCE_LEN = [200, 1000]                                     # enhance_waves: 41 frames
STREAM_LEN, STREAM_BLOCKS = 200, [70, 33, 97]                 # 8 frames, all of them due with the last block (the NAT row needs 6)


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
    return dict(maker=None, maker_kind=None, maker_nat=0, rows=0, windows=False, has_targ=False, preset=0, out=0, fwd=0, bunches=0,
                nat=0, post=0)


def _resident(st, pos, kind, rows, windows, has_targ):
    st.update(maker=pos, maker_kind=kind, maker_nat=st["nat"], rows=rows, windows=windows, has_targ=has_targ)


# What a call asks for beyond its data -- the score width, the target, the GV stage, the tracker, the kernel id -- is a function of
# (configuration, position) alone (choice), so a precondition takes the call's position too.
WIDTHS = (3, 5, 7)                                             # bp_eval_mix | bp_eval_mix_ext with 5 | with 7 score columns
NAT_MODES = ("static", "dynamic")
TIME_ITERS = (1, 2, 3)


def has_reverb(cfg):
    return cfg.id == "D"


def mask_col(cfg):
    """First column of the mask block in the net's output, or None on a net without one."""
    return None if cfg.ls[-1] == FEA_DIM else cfg.outs[0][1]


def post_settings(cfg):
    """What set_post cycles through: (GV on?, gate: None | (lo, hi, weight)).  A net without mask columns gets GV only."""
    if mask_col(cfg) is None:
        return [(False, None), (True, None)]
    return [(False, None), (True, None), (True, (0.3, 0.7, 0.5)), (False, (0.5, 0.5, 1.0))]


def gv_arrays(cfg):
    """(center, scale) of the GV setting: any finite centre and positive scale serve a bit-for-bit comparison."""
    rng = np.random.default_rng([cfg.index, 55])
    return rng.normal(10.0, 2.0, FEA_DIM).astype(np.float32), rng.uniform(0.6, 1.6, FEA_DIM).astype(np.float32)


def time_ids(cfg):
    """The kernel ids bp_time_kernel accepts on this net (0..2 need numlayers >= 4)."""
    return list(range(6)) if len(cfg.ls) >= 4 else [3, 4, 5]


def _mix(pos, salt, n):
    """A choice among n by position: a fixed integer hash, no state."""
    x = (pos * 2654435761 + salt * 40503 + 12345) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 2246822519) & 0xFFFFFFFF
    x ^= x >> 13
    return int(x % n)


def choice(cfg, pos, kind):
    """What the call at position pos asks for beyond its data."""
    if kind == "eval_mix":
        return dict(width=WIDTHS[_mix(pos, 1, 3)], masked=bool(_mix(pos, 2, 2)))
    if kind == "eval_mix_logmmse":
        return dict(width=WIDTHS[_mix(pos, 1, 3)], noise=(None, "spp")[_mix(pos, 3, 2)])
    if kind == "gv_mix":
        return dict(stage=("raw", "post")[_mix(pos, 4, 2)])
    if kind == "time_kernel":
        ids = time_ids(cfg)
        return dict(which=ids[_mix(pos, 5, len(ids))], iters=TIME_ITERS[_mix(pos, 6, len(TIME_ITERS))])
    return {}


def _pre_none(cfg, st, pos):
    return None


def _pre_resident_bunch(cfg, st, pos):
    """train_resident(0, B) and grads_resident(0): one bunch of whatever is resident."""
    if st["rows"] < cfg.B:
        return "range"                                         # frame range outside the resident chunk (checked first)
    if not st["has_targ"]:
        return "no targets"                                    # the call that made the chunk resident supplied no targets
    return None


_FAIL_RESIDENT_BUNCH = {"range": BP_ERR_ARG, "no targets": BP_ERR_STATE}


def _pre_set_forward(cfg, st, pos):
    return "bf16" if cfg.dtype == 1 else None                  # the bf16 forward has no row-invariant kernel


def _pre_eval_mix(cfg, st, pos):
    if st["post"] and mask_col(cfg) is not None and choice(cfg, pos, "eval_mix")["masked"]:
        return "mask target under post-processing"
    return None


def _pre_time_kernel(cfg, st, pos):
    if cfg.dtype == 1:
        return "bf16"                                          # (checked first)
    if st["rows"] < cfg.B or st["windows"]:
        return "no stacked chunk"
    return None


def _pre_profile_step(cfg, st, pos):
    return "bf16" if cfg.dtype == 1 else _pre_resident_bunch(cfg, st, pos)


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


def _ap_set_nat(cfg, st, pos):
    st["nat"] ^= 1


def _ap_set_post(cfg, st, pos):
    st["post"] = (st["post"] + 1) % len(post_settings(cfg))


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
    # (the mask target is refused under post-processing, which only set_post turns on: REACHED_BY)
    Kind("eval_mix", _pre_eval_mix, False, _ap_query_chunk("eval_mix", True, False, _q41), {"mask target under post-processing": BP_ERR_ARG}),
    Kind("grads", _pre_none, False, _ap_query_chunk("grads", False, True, query_rows), {}),
    # the gradient of the first bunch of WHATEVER is resident, stacked or window, legal or refused as train_resident(0, B) is; it
    # leaves the chunk, the weights and the dropout stream where they were
    Kind("grads_resident", _pre_resident_bunch, False, _ap_nothing, _FAIL_RESIDENT_BUNCH),
    # (only the last push has frames due: its 8 rows, fewer than either bunch, become the resident chunk)
    Kind("stream", _pre_none, False, _ap_query_chunk("stream", True, False, lambda cfg: frames_of(STREAM_LEN)), {}),
    Kind("set_forward", _pre_set_forward, False, _ap_set_forward, {"bf16": BP_ERR_ARG}),
    Kind("checkpoint", _pre_none, False, _ap_nothing, {}),
    # ---- NEW_KINDS: the two switches the handle gained behind those nineteen, the two calls that share the ev_* buffers with
    # bp_eval_mix, and the two measurement calls that bench.py makes on the handle it goes on measuring with
    # read by bp_train_mix: the replay repeats it
    Kind("set_nat", _pre_none, True, _ap_set_nat, {}),
    # "The log-MMSE calls, training and CV are unaffected.": the replay leaves it out, like set_forward
    Kind("set_post", _pre_none, False, _ap_set_post, {}),
    Kind("gv_mix", _pre_none, False, _ap_query_chunk("gv_mix", True, False, _q41), {}),
    Kind("eval_mix_logmmse", _pre_none, False, _ap_query_chunk("eval_mix_logmmse", True, False, _q41), {}),
    # no training and no query: the handle trains on like the replay, which never made the call
    Kind("time_kernel", _pre_time_kernel, False, _ap_nothing, {"bf16": BP_ERR_STATE, "no stacked chunk": BP_ERR_STATE}),
    # profile_step(0, 1) is one bunch: the replay runs train_resident(0, B) in its place (REPLAY_AS)
    Kind("profile_step", _pre_profile_step, True, _ap_train_resident, dict(_FAIL_RESIDENT_BUNCH, bf16=BP_ERR_STATE)),
])
NEW_KINDS = ["set_nat", "set_post", "gv_mix", "eval_mix_logmmse", "time_kernel", "profile_step"]
# query kinds that make a chunk WITH targets resident: the replay handle, which leaves queries out, loads their chunk when a
# later train_resident trains on it
LOADABLE = ("mix_features", "grads")
REPLAY_AS = {"profile_step": "train_resident"}
# non-training kinds that are no query: nothing to compare with a fresh handle
NO_FRESH = ("checkpoint", "set_forward", "set_post", "time_kernel")
READS_NAT = ("train_mix", "cv_mix", "mix_features", "enhance", "eval_mix", "gv_mix", "stream")
READS_POST = ("enhance", "eval_mix", "gv_mix", "stream")      # (gv_mix: at stage POST)
TRAINING_KINDS = [k for k, v in KINDS.items() if v.training and k not in ["preset", "set_output"] + NEW_KINDS]
# A refusal that only arises behind a call of another kind: reason -> that kind.  The table without NEW_KINDS is a restriction of
# the whole one: its walks never reach set_post, so `post` stays 0 and the precondition of eval_mix is None on every one of them
# (tests/test_walk_digests.py: their steps are what they were when eval_mix had no precondition).
REACHED_BY = {"mask target under post-processing": "set_post"}


def table(kinds):
    """KINDS restricted to `kinds`: a refusal that no walk over them can reach is dropped, and a precondition without refusals is none."""
    out = collections.OrderedDict()
    for n in kinds:
        fail = {why: st for why, st in KINDS[n].fail.items() if REACHED_BY.get(why, n) in kinds}
        out[n] = KINDS[n]._replace(pre=KINDS[n].pre if fail else _pre_none, fail=fail)
    return out


_LEAVES = {}


def leaves(kind):
    """(window chunk?, targets?) of what a call of `kind` leaves resident: the kind's own update, asked once."""
    if kind not in _LEAVES:
        st = fresh_state()
        KINDS[kind].apply(CONFIGS[0], st, 0)
        _LEAVES[kind] = (st["windows"], st["has_targ"])
    return _LEAVES[kind]


# ------------------------------------------------------------------ the families
# Closed: one closed walk that takes every ordered pair of its nodes exactly once, cut into `pieces` GPU tests.  A node is a kind, with
# a size where the family's calls have one (`sizes`: the sizes the walk takes) and the handle's noise-aware mode (`modes`) where the
# walk switches it.  kinds None: every kind of the configuration.  seed: the tail of the seed behind the configuration's index.
Closed = collections.namedtuple("Closed", "fid pieces walk seed kinds sizes modes")
# Built: a walk by construction, `calls` a function of the configuration.  walk: the walk number, which selects the data.
Built = collections.namedtuple("Built", "wid walk calls")
# name         the key of the family (tests/golden/walk_digests.json)
# kinds        the kinds its walks draw on; configs: its configurations
# sizes        {kind: its sizes} where calls carry a size (a call is then (pos, kind, size), else (pos, kind)); layer: the module that
#              knows what a size is (tests/size_model.py); cap: max_chunk_frames of every handle
# choice       a call's data carries choice(...)
# closed, built, then n_random seeded walks of RANDOM_LEN calls: ids random_id + number, seeds random_seed + number, walk numbers
#              random_no + number
# corpus_seeds, twins   (sized families) the seeds of the recordings and of the entries behind them (None: the same stream goes on);
#              whether the corpus carries reverberated twins of those entries on D
# gpu_file, gpu_test, timed   where the walks run, and whether the record of a run holds its seconds
Family = collections.namedtuple("Family", "name kinds configs sizes layer cap choice closed built n_random random_id random_seed random_no "
                                          "corpus_seeds twins gpu_file gpu_test timed")
RANDOM_LEN = 60
# (the seeds of EXTENDED: the first at which every claim of tests/test_sequence_coverage.py about its walks holds in all configurations)
X_SEED, X_CLOSED_SEED = 3000, 17
N_TIME_TAIL = 16


def measure_walk(cfg):
    """The measurement calls where they succeed, which a seeded walk reaches by luck alone (bp_time_kernel wants a stacked chunk of a
    bunch, bp_profile_step one with targets): each behind a chunk it accepts and in front of every training kind, then a row of
    bp_time_kernel calls, whose kernel id follows the position, behind one stacked chunk."""
    out = []
    for t in TRAINING_KINDS:
        out += ["train", "time_kernel", t, "checkpoint", "train_windows", "profile_step", t, "checkpoint"]
    out += ["upload_train"] + ["time_kernel"] * N_TIME_TAIL + ["train_resident", "checkpoint"]
    return list(enumerate(out))


# Pieces of a closed walk, each a GPU test of its own from a fresh subject and replay.  A whole closed walk of WALK takes about two
# seconds on an MI355X (362 calls on three handles and some 200 fresh ones), one of EXTENDED (625 pairs, 576 on B) 0.8 to 0.9 seconds in
# the run whose figures are committed (3.0 to 3.4 on another day, measured in two halves), under the ten it may take: ONE piece each.
# With more, a piece starts with the call that the piece before it ended with, so that no pair is dropped at a cut (cut).
WALK = Family(name="walk", kinds=tuple(k for k in KINDS if k not in NEW_KINDS), configs=CONFIGS[:3], sizes=None, layer=None, cap=CAP,
              choice=False, closed=[Closed("closed", pieces=1, walk=0, seed=(7,), kinds=None, sizes=None, modes=None)], built=[],
              n_random=4, random_id="random", random_seed=1000, random_no=1, corpus_seeds=None, twins=False,
              gpu_file="test_sequence_gpu.py", gpu_test="test_walk", timed=False)
# (the walk numbers lie behind WALK's)
EXTENDED = Family(name="extended", kinds=tuple(KINDS), configs=CONFIGS, sizes=None, layer=None, cap=CAP,
                  choice=True, closed=[Closed("xclosed", pieces=1, walk=10, seed=(X_CLOSED_SEED,), kinds=None, sizes=None, modes=None)],
                  built=[Built("xmeasure", 11, measure_walk)],
                  n_random=4, random_id="xrandom", random_seed=X_SEED, random_no=12, corpus_seeds=None, twins=False,
                  gpu_file="test_sequence_gpu.py", gpu_test="test_extended_walk", timed=True)


def kinds_of(fam, cfg):
    """set_output applies only where the net has logistic columns."""
    return [k for k in fam.kinds if k != "set_output" or len(cfg.outs) > 1]


Step = collections.namedtuple("Step", "pos kind size status before after")


def run_model(fam, cfg, calls, st=None):
    """The model over the calls of a walk from a fresh handle: one Step per call with the expected status and the model state before
    and after it (size None where the call has none).  A sized call is refused for its size first (the capacity is checked with the
    plan, before the switches are read); what it leaves resident and trains is its shape's."""
    st = fresh_state() if st is None else dict(st)
    out = []
    for call in calls:
        pos, kind, size = call if fam.sizes else call + (None,)
        k = KINDS[kind]
        before = dict(st)
        why = k.pre(cfg, st, pos)
        status = BP_OK if why is None else k.fail[why]
        if fam.sizes and kind in fam.sizes:
            s = fam.layer.shape(cfg, kind, size)
            if not s.ok:
                status = BP_ERR_ARG
            elif status == BP_OK:
                _resident(st, pos, kind, s.resident, *leaves(kind))
                st["bunches"] += s.bunches
        elif status == BP_OK:
            k.apply(cfg, st, pos)
        out.append(Step(pos, kind, size, status, before, dict(st)))
    return out


def idle(fam, cfg, step):
    """A successful training call that trains nothing (size Z)."""
    return step.size is not None and KINDS[step.kind].training and step.status == BP_OK and fam.layer.shape(cfg, step.kind, step.size).bunches == 0


# ------------------------------------------------------------------ the walks
def _circuit(K, seed):
    """An Eulerian circuit of the complete directed graph with loops on K nodes, from node 0 (Hierholzer; the order of each node's
    edges from a seeded shuffle).  K * K + 1 entries, the last one the first again."""
    rng = np.random.default_rng(seed)
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
    return circuit


def closed_of(fam, fid):
    return [c for c in fam.closed if c.fid == fid][0]


def n_pieces(fam):
    return collections.OrderedDict((c.fid, c.pieces) for c in fam.closed)


def nodes(fam, cfg, fid):
    """The nodes of a closed walk: (kind,), (kind, size) or (kind, size, mode)."""
    c = closed_of(fam, fid)
    ks = kinds_of(fam, cfg) if c.kinds is None else c.kinds
    if not fam.sizes:
        return [(k,) for k in ks]
    ns = [(k, z) for k in ks for z in fam.sizes[k] if z in c.sizes]
    return [n + (m,) for n in ns for m in c.modes] if c.modes else ns


def closed_walk(fam, cfg, fid, salt=None):
    """The nodes of one closed walk that takes every ordered pair of them exactly once (salt: in place of the last word of the seed)."""
    c, ns = closed_of(fam, fid), nodes(fam, cfg, fid)
    tail = c.seed if salt is None else c.seed[:-1] + (salt,)
    return [ns[i] for i in _circuit(len(ns), [cfg.index] + list(tail))]


def cut(walk, P):
    """P pieces of a closed walk, [(index in the walk,) + node, ...] each: a piece starts with the entry the one before it ended with."""
    n = len(walk) - 1
    cuts = [round(i * n / P) for i in range(P + 1)]
    return [[(p,) + walk[p] for p in range(cuts[i], cuts[i + 1] + 1)] for i in range(P)]


def with_modes(seq, nat=0):
    """[(node index, kind, size, mode)] -> calls: pos = 2 * index for the node, 2 * index - 1 for the set_nat in front of it where the
    node's mode is not the handle's (a stream opens inside its call, so behind the set_nat)."""
    out = []
    for i, k, z, m in seq:
        if m != nat:
            out.append((2 * i - 1, "set_nat", None))
            nat = m
        out.append((2 * i, k, z))
    return out


def pieces(fam, cfg, fid, n_pieces=None, salt=None):
    """The calls per piece, each from a fresh handle (static mode); pos is the index in the closed walk (it selects the data)."""
    c = closed_of(fam, fid)
    ps = cut(closed_walk(fam, cfg, fid, salt), c.pieces if n_pieces is None else n_pieces)
    return [with_modes(p) for p in ps] if c.modes else ps


def piece_ids(fam, fid, n_pieces=None):
    P = closed_of(fam, fid).pieces if n_pieces is None else n_pieces
    return [fid if P == 1 and not fam.sizes else "%s%d" % (fid, i) for i in range(P)]


def piece_nodes(fam, cfg, fid, n_pieces=None):
    """The nodes per piece as the MODEL runs them (where the walk switches the mode: with the handle's); a node of one field is the field."""
    ps = pieces(fam, cfg, fid, n_pieces)
    if closed_of(fam, fid).modes:
        return [[(s.kind, s.size, s.before["nat"]) for s in run_model(fam, cfg, p) if s.kind != "set_nat"] for p in ps]
    return [[c[1] if len(c) == 2 else c[1:] for c in p] for p in ps]


def pair_table(fam, cfg, fid, n_pieces=None):
    """(node, next node) -> the ids of the pieces that run it."""
    out = {}
    for wid, p in zip(piece_ids(fam, fid, n_pieces), piece_nodes(fam, cfg, fid, n_pieces)):
        for a, b in zip(p, p[1:]):
            out.setdefault((a, b), []).append(wid)
    return out


def random_walk(fam, cfg, seed):
    """A kind of the configuration at random; where calls have a size, then one of its sizes (OVER among them)."""
    ks = kinds_of(fam, cfg)
    rng = np.random.default_rng([cfg.index, fam.random_seed + seed])
    out = []
    for p in range(RANDOM_LEN):
        call = (p, ks[int(rng.integers(len(ks)))])
        if fam.sizes:
            zs = fam.sizes.get(call[1], [None])
            call += (zs[int(rng.integers(len(zs)))],)
        out.append(call)
    return out


def walk_ids(fam, cfg):
    return ([w for c in fam.closed for w in piece_ids(fam, c.fid)] + [b.wid for b in fam.built] +
            ["%s%d" % (fam.random_id, s) for s in range(fam.n_random)])


def walk_calls(fam, cfg, wid):
    """(walk number for the data, calls) of one walk id."""
    for c in fam.closed:
        if wid in piece_ids(fam, c.fid):
            return c.walk, pieces(fam, cfg, c.fid)[piece_ids(fam, c.fid).index(wid)]
    for b in fam.built:
        if wid == b.wid:
            return b.walk, b.calls(cfg)
    s = int(wid[len(fam.random_id):])
    return fam.random_no + s, random_walk(fam, cfg, s)


def all_walks(fam, cfg):
    return [(wid,) + walk_calls(fam, cfg, wid) for wid in walk_ids(fam, cfg)]


def test_id(fam, cfg, wid):
    return "tests/%s::%s[%s-%s]" % (fam.gpu_file, fam.gpu_test, cfg.id, wid)


def gpu_tests(fam):
    return [test_id(fam, c, w) for c in fam.configs for w in walk_ids(fam, c)]


# ------------------------------------------------------------------ data
def recordings(cfg, seed):
    """(clean, noise, mean and inv_std from one seeded stream; the stream)."""
    rng = np.random.default_rng([cfg.index, seed])
    clean = [(rng.normal(size=n) * 3000.0).astype(np.float32) for n in CLEAN_LEN]
    noise = [(rng.normal(size=n) * 1500.0).astype(np.float32) for n in NOISE_LEN]
    mean = rng.normal(10.0, 2.0, FEA_DIM).astype(np.float32)
    inv_std = rng.uniform(0.2, 0.5, FEA_DIM).astype(np.float32)
    cor = dict(clean=clean, noise=noise, mean=mean, inv_std=inv_std)
    if has_reverb(cfg):                                        # also the responses, the pairs and the MFCC setting
        rir_rng = np.random.default_rng([cfg.index, 98])
        rirs = []
        for n in RIR_TAPS:
            h = (rir_rng.normal(size=n) * np.exp(-np.arange(n) / 8.0)).astype(np.float32)
            h[3] = 3.0                                         # the direct path
            rirs.append(h)
        cor.update(rirs=rirs, pair_clean=[c for c, _ in REVERB_PAIRS], pair_rir=[r for _, r in REVERB_PAIRS], reverb_target=REVERB_TARGET,
                   early_taps=EARLY_TAPS, aux=dict(AUX))
    return cor, rng


def corpus(fam, cfg):
    return fam.layer.sized_corpus(fam, cfg) if fam.sizes else recordings(cfg, 99)[0]


def plan_train_clean(cfg):
    """train_clean with the first long sentence taken from the room (entry 4 is sentence 3 reverberated: the same frames)."""
    c = train_clean(cfg)
    return [4] + c[1:] if has_reverb(cfg) else c


def plan_query_clean(cfg):
    return [5, 3] if has_reverb(cfg) else QUERY_CLEAN             # (entry 5 is sentence 0 reverberated)


def _targets(cfg, rng, n):
    sL = cfg.ls[-1]
    t = rng.normal(size=(n, sL)).astype(np.float32)
    if len(cfg.outs) > 1:                                      # the logistic columns: targets in [0, 1]
        lo = cfg.outs[0][1]
        t[:, lo:] = rng.uniform(size=(n, sL - lo)).astype(np.float32)
    return t


def _stacked(cfg, rng, n):
    return dict(x=rng.normal(size=(n, cfg.ls[0])).astype(np.float32), t=_targets(cfg, rng, n))


def _windows(cfg, rng, n):
    nf = n + 7
    ws = rng.integers(0, nf - CONTEXT + 1, n).astype(np.int32)
    return dict(fea=rng.normal(size=(nf, FEA_DIM)).astype(np.float32), targ_frames=_targets(cfg, rng, nf), win_start=ws,
                targ_frame=(ws + TARG_OFFSET).astype(np.int32), nat=rng.normal(size=(2, FEA_DIM)).astype(np.float32),
                nat_row=rng.integers(0, 2, n).astype(np.int32))


def mixtures(rng, clean):
    """Rows (clean, noise, offset, snr_db) of a mixture plan."""
    out = []
    for c in clean:
        nz = int(rng.integers(len(NOISE_LEN)))
        out.append((int(c), nz, int(rng.integers(NOISE_LEN[nz])), float(SNRS[int(rng.integers(len(SNRS)))])))
    return out


MIX_QUERIES = ("cv_mix", "mix_features", "eval_mix", "gv_mix", "eval_mix_logmmse")


def call_data(fam, cfg, walk, pos, kind, size=None):
    """What the call at position pos of walk number `walk` is made with: where the family's data carry it, what the call asks for
    beyond its data (choice); then the arrays and plans, a sized call's from the family's layer."""
    d = choice(cfg, pos, kind) if fam.choice else {}
    if fam.sizes:
        return dict(d, **fam.layer.sized_data(fam, cfg, walk, pos, kind, size)) if kind in fam.sizes else d
    rng = np.random.default_rng([cfg.index, walk, pos])
    if kind in ("train", "upload_train"):
        d.update(_stacked(cfg, rng, train_rows(cfg)))
    elif kind in ("forward", "cv", "grads"):
        d.update(_stacked(cfg, rng, query_rows(cfg)))
    elif kind == "train_windows":
        d.update(_windows(cfg, rng, train_rows(cfg)))
    elif kind == "cv_windows":
        d.update(_windows(cfg, rng, query_rows(cfg)))
    elif kind == "train_mix":
        d.update(plan=mixtures(rng, plan_train_clean(cfg)), order=MX.shuffle(1 + pos, 10 * walk + cfg.index, mix_rows(train_clean(cfg))))
    elif kind in MIX_QUERIES:
        d.update(plan=mixtures(rng, plan_query_clean(cfg)))
    elif kind == "enhance":
        d.update(sentences=[(rng.normal(size=n) * 3000.0).astype(np.float32) for n in ENHANCE_LEN])
    elif kind == "stream":
        x = (rng.normal(size=STREAM_LEN) * 3000.0).astype(np.float32)
        d.update(blocks=np.split(x, np.cumsum(STREAM_BLOCKS)[:-1]))
    return d


# ------------------------------------------------------------------ every entry point that takes a handle
# include/bp_c_api.h function (first parameter bp_handle *) -> the kinds of KINDS whose call (tests/walk_harness.py) makes it, or
# (one line of reason, the test file that holds it instead).  tests/test_sequence_coverage.py parses the header and fails on a
# symbol that is not here, on a kind that is not in the table, and on a kind no entry names.
API = collections.OrderedDict([
    ("bp_destroy", ("every walk closes its handles: nothing is carried behind it", "tests/test_mem_gpu.py", ".close()")),
    ("bp_set_hyper", ["preset"]),
    ("bp_set_output", ["set_output"]),
    ("bp_set_forward", ["set_forward"]),
    ("bp_train_chunk", ["train"]),
    ("bp_cv_chunk", ["cv"]),
    ("bp_forward", ["forward"]),
    ("bp_get_weights", ["checkpoint"]),
    ("bp_get_deltas", ["checkpoint"]),
    ("bp_upload_chunk", ["upload_train", "grads"]),
    ("bp_fill_chunk_synthetic", ["grads", "grads_resident"]),   # (the fresh handle's way to the subject's dropout position)
    ("bp_train_resident", ["upload_train", "train_resident"]),
    ("bp_sync", ("a host wait on the handle's stream: it changes nothing", "tests/test_gpu_parity.py", ".sync()")),
    ("bp_train_resident_masked", ("its own parity tests; its refusals stand beside train_resident's", "tests/test_sequence_gpu.py")),
    ("bp_upload_chunk_windows", ["grads_resident", "train_resident"]),   # (load: the chunk a window call left, on a fresh handle)
    ("bp_train_chunk_windows", ["train_windows"]),
    ("bp_cv_chunk_windows", ["cv_windows"]),
    ("bp_forward_windows", ("bp_cv_chunk_windows without targets: the same upload, the same forward", "tests/test_infer_gpu.py")),
    ("bp_enhance_waves", ["enhance"]),
    ("bp_set_mix_corpus", ("the construction of every walked handle", "tests/walk_harness.py", "g.set_mix_corpus(")),
    ("bp_train_mix", ["train_mix"]),
    ("bp_cv_mix", ["cv_mix"]),
    ("bp_mix_features", ["mix_features"]),
    ("bp_set_mix_aux", ("configuration D's construction: the MFCC columns, set before the corpus", "tests/walk_harness.py", "g.set_mix_aux(")),
    ("bp_set_mix_reverb", ("configuration D's construction: the derived entries its plans draw on", "tests/walk_harness.py", "g.set_mix_reverb(")),
    ("bp_eval_mix", ["eval_mix"]),
    ("bp_eval_mix_ext", ["eval_mix"]),
    ("bp_eval_mix_logmmse", ["eval_mix_logmmse"]),
    ("bp_eval_mix_logmmse_ext", ["eval_mix_logmmse"]),
    ("bp_eval_mix_logmmse_nt", ["eval_mix_logmmse"]),
    ("bp_stream_open", ["stream"]),
    ("bp_set_nat", ["set_nat"]),
    ("bp_set_post", ["set_post"]),
    ("bp_gv_mix", ["gv_mix"]),
    ("bp_grads_resident", ["grads", "grads_resident"]),
    ("bp_grad_floats", ["grads", "grads_resident"]),
    ("bp_grad_layout", ["grads", "grads_resident"]),
    ("bp_read_grads", ["grads", "grads_resident"]),
    ("bp_read_layer_output", ("a pure read of the last bunch's activations", "tests/test_gpu_parity.py")),
    # (the life of an attachment: tests/test_dp_life_gpu.py starts tests/dp_life_worker.py)
    ("bp_dp_attach", ("data-parallel handles; the binding attaches through bp_dp_attach_ex", "tests/dp_life_worker.py", "dp_attach(")),
    ("bp_dp_attach_ex", ("data-parallel handles: the life of an attachment", "tests/dp_life_worker.py", "dp_attach(")),
    ("bp_dp_detach", ("data-parallel handles: the life of an attachment", "tests/dp_life_worker.py")),
    ("bp_dp_info", ("a pure read of the attachment", "tests/dp_life_worker.py")),
    ("bp_dp_peer_info", ("a pure read of the attachment", "tests/dp_worker.py")),
    ("bp_dp_handoff", ("a pure read of the attachment", "tests/test_dp_native.py")),
    ("bp_dp_barrier", ("host-side, over the rendezvous block", "bench.py")),
    ("bp_dp_allgather", ("host-side, over the rendezvous block", "bench.py", "dp_allgather_f64(")),
    ("bp_last_train_ms", ("a pure read of the two events around the last bunch loop; no test makes it", "tools/bench_bf16.py")),
    ("bp_time_kernel", ["time_kernel"]),
    ("bp_profile_step", ["profile_step"]),
    ("bp_measure_peaks", ("it touches only the handle's stream and allocates 2 GiB", "bench.py")),
])


def api_problems(api, kinds, header_text):
    """What is wrong between the header's handle functions, the API map and the kind table, each problem by name."""
    import re
    flat = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    fns = re.findall(r"\b(bp_\w+)\s*\(\s*bp_handle\s*\*", flat)
    out = ["unclassified entry point %s" % f for f in fns if f not in api]
    out += ["%s is classified but the header has no such handle function" % f for f in api if f not in fns]
    named = set()
    for f, v in api.items():
        if isinstance(v, list):
            named.update(v)
            out += ["%s names the kind %s, which the table does not have" % (f, k) for k in v if k not in kinds]
    out += ["no entry point names the kind %s" % k for k in kinds if k not in named]
    return out


# ------------------------------------------------------------------ the figures of a GPU run
# The committed records (profiles/<name>_parity_numbers.json) and the GPU files whose entries each holds.  `source` is the text the
# record was committed with: it names the command line of its day.
RECORDS = collections.OrderedDict([
    ("sequence", (("test_sequence_gpu.py", "test_dp_life_gpu.py"),
                  "a -m gpu run of tests/test_sequence_gpu.py and tests/test_dp_life_gpu.py on an MI355X; "
                  "`python tests/sequence_model.py numbers <parity JSON> <out>` behind it",
                  "bit for bit: words_differing == 0 in every entry (the life against one rank: 1e-5)")),
    ("size", (("test_size_gpu.py",),
              "a -m gpu run of tests/test_size_gpu.py on an MI355X; `python tests/size_model.py numbers <parity JSON> <out>` behind it",
              "bit for bit: words_differing == 0 in every entry")),
    ("xsize", (("test_xsize_gpu.py",),
               "a -m gpu run of tests/test_xsize_gpu.py on an MI355X; `python tests/xsize_model.py numbers <parity JSON> <out>` behind it",
               "bit for bit: words_differing == 0 in every entry")),
])


def numbers(record, parity):
    """The entries of a session's parity JSON (conftest.py) that belong in the record of that name."""
    files, source, bar = RECORDS[record]
    return {"source": source, "bar": bar, "tests": {k: v for k, v in sorted(parity["tests"].items()) if any(f in k for f in files)}}


if __name__ == "__main__":
    import json
    import sys
    if len(sys.argv) == 5 and sys.argv[1] == "numbers":         # numbers <sequence | size | xsize> <parity JSON> <out>
        json.dump(numbers(sys.argv[2], json.load(open(sys.argv[3]))), open(sys.argv[4], "w"), indent=1, sort_keys=True)
    else:
        for cfg in WALK.configs:
            print(cfg.id, " ".join(k for k, in closed_walk(WALK, cfg, "closed")))
