"""A size axis on top of tests/sequence_model.py: the same handle, the same call kinds, calls of CHANGING size.  Imports neither the
package nor a GPU; tests/test_size_coverage.py checks everything in here on any machine, tests/test_size_gpu.py runs the walks.

What sizes reach and constant sizes never do: the grow-only buffers of a handle (Buf::grow, csrc/bp_mem.h) are regrown -- the
streams named at the call site are synchronised, the old block is freed, n + n/4 + 4096 bytes of UNZEROED memory come back -- and a
small call runs in buffers whose tails hold a larger call's data.  BUFFERS below is the table of those buffers, written from the
call sites (SITES): which kinds size a buffer and how many bytes a call asks for.  The families of kinds that share state, the size
class L ("large enough that every buffer is regrown behind an M call") and the regrow / shrink claims of the coverage test are all
computed from that table and the policy; nothing of it needs a device.

Size classes of a call (SIZES), rows per call with FEA_DIM 33, the configurations and bunch sizes of sequence_model, CAP 1024:
  Z     fewer rows than a bunch: one row (stacked and window kinds), one sentence of one sample (mix, enhance, eval, stream kinds).
        A training call of size Z trains nothing.
  ONE   exactly B rows: one bunch, an odd count
  M     the size of sequence_model's walks: two bunches and a part (training), B + 3 rows or 41 frames (queries)
  L     nb bunches and half a bunch, nb the smallest odd count >= 3 at which every buffer the kind sizes, and that the policy lets
        regrow at all, is regrown behind an M call of that kind (large()); the sentence kinds take more sentences AND one long one
  FULL  exactly CAP rows
  OVER  CAP + 1 rows: BP_ERR_ARG, the model state stays as it was
The gradient query has no Z: its gradient is that of one whole bunch (NO_Z).

Dye: the query kinds at L and FULL carry NaN in their input (rows, PCM samples, the nat rows of window chunks), so every buffer they
touch is full of NaN when the next, smaller call runs, and a leak of remains shows as NaN, not as a small error.  Training kinds
stay finite.  The two queries that leave a chunk WITH targets (sequence_model.LOADABLE) keep the rows that a train_resident or
grads_resident behind them reads finite -- the first B + 3 rows of the gradient upload, the first mixture of mix_features -- so that
the net stays finite; everything behind those rows is NaN.  No entry point refuses non-finite samples or rows by design (only SNRs,
lc_db and impulse-response taps are checked), so FINITE_DYE, the kinds dyed with 3e38-scale values instead, is empty."""
import collections

import numpy as np

import mix_np as MX
import sequence_model as SM
import stream_np as ST

CAP = 1024
SIZES = ("Z", "ONE", "M", "L", "FULL", "OVER")
GOOD = SIZES[:-1]
D, HOP, CTX = SM.FEA_DIM, SM.HOP, SM.CONTEXT
STACKED = ("train", "upload_train", "forward", "cv", "grads")
WINDOWS = ("train_windows", "cv_windows")
MIXED = ("train_mix", "cv_mix", "mix_features", "eval_mix")
SENTENCES = MIXED + ("enhance", "stream")
SIZED = [k for k in SM.KINDS if k in STACKED + WINDOWS + SENTENCES]
UNSIZED = [k for k in SM.KINDS if k not in SIZED]
NO_Z = {"grads": "the gradient is that of one whole bunch: a chunk of fewer rows has none"}
DYED = ("L", "FULL")
FINITE_DYE = ()                                                # kinds whose entry point refuses non-finite input by design: none
N_SHORT, SHORT_T = 34, 5                                       # L of the sentence kinds: 34 sentences of 5 frames and one long one
N_NAT_L = 40                                                   # nat rows of a window chunk at L and FULL (M: 2)
STREAM_L = dict(n_chan=4, max_push=16384, per_block=4000, pushes=2)


def sizes_of(kind):
    return [s for s in SIZES if not (s == "Z" and kind in NO_Z)] if kind in SIZED else [None]


def sl_of(cfg):
    return cfg.ls[-1]


def len_of(T):
    """Samples of a sentence of T frames (T = (n - 1) // HOP + 2); T = 2: ONE sample."""
    return 1 if T == 2 else (T - 2) * HOP + 7


# ------------------------------------------------------------------ the allocation policy (csrc/bp_mem.h; out_chunk_reserve: csrc/bp_step.hip)
def grown(n):
    """Buf::grow: no growth while n <= bytes, else n + n/4 + 4096 bytes."""
    return n + n // 4 + 4096


def grown_frames(n):
    """out_chunk_reserve (frames, not bytes): no growth while n <= out_chunk_frames, else n + n/4 + 64 frames."""
    return n + n // 4 + 64


POLICY = {"grow": grown, "frames": grown_frames}


def al256(b):
    return (b + 255) & ~255


# ------------------------------------------------------------------ the shape of a call
# n: samples of the chunk (frames); rows: staged rows; nf: raw frames of a window upload; n_sent: sentences / mixtures / channels;
# n_nat: nat rows; uses: how many times the call takes a window staging set (a stream: its pushes with frames due); bunches: what a
# training call trains; open_frames: what a stream reserves of out_chunk when it opens (also when its push is refused); ok: not OVER
Shape = collections.namedtuple("Shape", "kind size ok n rows nf n_sent n_nat uses bunches resident open_frames T pushes")


def _row_count(cfg, kind, size):
    B = cfg.B
    if size == "Z":
        return 1
    if size == "ONE":
        return B
    if size == "M":
        return SM.train_rows(cfg) if SM.KINDS[kind].training else SM.query_rows(cfg)
    if size == "FULL":
        return CAP
    if size == "OVER":
        return CAP + 1
    raise AssertionError(size)


def _sentence_T(cfg, kind, size, nb=None):
    """Frames per sentence of a sentence kind."""
    B = cfg.B
    if size == "Z":
        return [2]
    if size == "ONE":
        return [B]
    if size == "M":
        if kind == "train_mix":
            return [SM.frames_of(SM.CLEAN_LEN[c]) for c in SM.train_clean(cfg)]
        if kind == "enhance":
            return [SM.frames_of(n) for n in SM.ENHANCE_LEN]
        if kind == "stream":
            return [SM.frames_of(SM.STREAM_LEN)]
        return [SM.frames_of(SM.CLEAN_LEN[c]) for c in SM.QUERY_CLEAN]
    if size == "L":                                            # the long sentence first: mix_features keeps it finite
        frames = nb * B + B // 2
        return [frames - N_SHORT * SHORT_T] + [SHORT_T] * N_SHORT
    if kind == "stream":                                       # one channel, one push: T + CTX - 1 rows
        return [CAP - (CTX - 1) + (1 if size == "OVER" else 0)]
    if size == "FULL":                                         # two sentences: frames + 2 (CTX - 1) = CAP rows
        return [(CAP - 2 * (CTX - 1)) // 2] * 2
    return [CAP + 1 - (CTX - 1)]                               # OVER: one sentence, CAP + 1 rows


def _stream_pushes(cfg, size, T):
    """(n_chan, max_push, [[samples per channel] per push], [[end flag per channel] per push])."""
    if size == "M":
        return 1, 256, [[b] for b in SM.STREAM_BLOCKS], [[i == len(SM.STREAM_BLOCKS) - 1] for i in range(len(SM.STREAM_BLOCKS))]
    if size == "L":                                            # four channels, two pushes near max_push_samples, all ending in the second
        nc, per = STREAM_L["n_chan"], STREAM_L["per_block"]
        blocks = [[per + 7 * c for c in range(nc)], [per + 90 - 11 * c for c in range(nc)]]
        assert all(sum(b) <= STREAM_L["max_push"] for b in blocks)
        return nc, STREAM_L["max_push"], blocks, [[False] * nc, [True] * nc]
    n = len_of(T[0])                                           # Z, ONE, FULL, OVER: one channel, the whole sentence in one push
    return 1, max(n, 256), [[n]], [[True]]


def _stream_due(pushes, ends, nc):
    """Frames due per push, per channel (stream_np.counts; every net here has the noise-aware block)."""
    got, out = [0] * nc, []
    for blk, e in zip(pushes, ends):
        due = []
        for c in range(nc):
            f0 = ST.counts(D, CTX, SM.TARG_OFFSET, True, got[c], False)[1]
            got[c] += blk[c]
            due.append(ST.counts(D, CTX, SM.TARG_OFFSET, True, got[c], e[c])[1] - f0)
            if e[c]:
                got[c] = 0
        out.append(due)
    return out


def shape(cfg, kind, size, nb=None):
    """The Shape of a call; nb: the bunch count of L (default: large(cfg, kind))."""
    if kind not in SIZED:
        return Shape(kind, None, True, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None)
    B, ok = cfg.B, size != "OVER"
    if size == "L" and nb is None:
        nb = large(cfg, kind)
    training = SM.KINDS[kind].training
    if kind in STACKED + WINDOWS:
        n = nb * B + B // 2 if size == "L" else _row_count(cfg, kind, size)
        bunches = n // B if training else 0
        if kind == "upload_train" and n >= 2 * B:
            bunches += 1                                       # train_resident(B, B) in front of train_resident(0, every whole bunch)
        win = kind in WINDOWS
        return Shape(kind, size, ok, n, n, n + 7 if win else 0, 0, (N_NAT_L if size in DYED else 2) if win else 0, 1 if win else 0,
                     bunches if ok else 0, n, 0, None, None)
    T = _sentence_T(cfg, kind, size, nb)
    if kind == "stream":
        nc, max_push, pushes, ends = _stream_pushes(cfg, size, T)
        due = _stream_due(pushes, ends, nc)
        if size == "L":
            T = [sum(p[c] for p in due) for c in range(nc)]
        per_push = [sum(d) for d in due]
        rows = max(sum(x + CTX - 1 for x in d if x > 0) for d in due)
        open_frames = min(max_push // HOP + 3 * nc + nc * (CTX + 6), CAP) + nc * B
        last = [p for p in per_push if p > 0][-1]
        return Shape(kind, size, ok, max(per_push), rows, 0, nc, nc, sum(1 for p in per_push if p > 0) if ok else 0, 0, last, open_frames,
                     T, (nc, max_push, pushes, ends))
    n, ns = sum(T), len(T)
    return Shape(kind, size, ok, n, n + ns * (CTX - 1), 0, ns, ns, 1, n // B if training and ok else 0, n, 0, T, None)


# ------------------------------------------------------------------ the buffers
# name -> (member: the Buf member or array the text scan finds; policy: "grow" (Buf::grow), "frames" (out_chunk_reserve, in frames),
# "fixed" (dev_alloc: sized by the capacity once and zero-filled; it never regrows, a smaller call still runs in a larger one's
# remains), slots: 2 where two blocks alternate per use (the staging sets: wcur; the pinned input blocks: pin_cur); site: SITES key;
# ask: {kind: Shape -> bytes (frames for "frames") the call asks for}; a kind that asks for 0 bytes does not size the buffer)
Buffer = collections.namedtuple("Buffer", "member policy slots site ask")


def _ask(kinds, fn):
    return collections.OrderedDict((k, fn) for k in kinds)


def _merge(*parts):
    out = collections.OrderedDict()
    for p in parts:
        out.update(p)
    return out


def _mix_in_bytes(s):
    """Call::bytes of plan_call (csrc/bp_mix.hip): F | Fs | clean | noise | offset | snr | order."""
    m = s.n_sent
    return 2 * al256((m + 1) * 4) + 2 * al256(m * 4) + al256(m * 8) + al256(m * 4) + al256(s.n * 4)


def _wave_in_bytes(s):
    """WaveIn::bytes (csrc/bp_wave.hip): F | mean | inv_std | window | twiddles | padded PCM."""
    return al256((s.n_sent + 1) * 4) + 2 * al256(D * 4) + al256(2 * HOP * 4) + al256((HOP + 1) * 8) + al256((s.n + s.n_sent) * HOP * 4)


_pcm = lambda s: (s.n + s.n_sent) * HOP * 4                   # segs * hop * 4: a sentence of T frames takes T + 1 segments
_WSET = WINDOWS + SENTENCES
_FWD = ("forward", "cv", "cv_windows", "cv_mix", "enhance", "eval_mix", "stream")
_out_frames = lambda s: max(s.n if s.ok else 0, s.open_frames)

BUFFERS = collections.OrderedDict([
    ("stacked pair", Buffer("allocs", "fixed", 2, "dev_alloc", _ask(STACKED, lambda s: s.n))),
    # (the window kinds stage through the tiles too: every pair of them is in the staging sets' family)
    ("stage tiles", Buffer("allocs", "fixed", 2, "dev_alloc", _ask(("train", "upload_train", "grads"), lambda s: s.n))),
    ("wset.r[0]", Buffer("r", "grow", 2, "wset_reserve", _merge(_ask(WINDOWS, lambda s: s.nf * D * 4), _ask(SENTENCES, lambda s: s.rows * D * 4)))),
    ("wset.r[1]", Buffer("r", "grow", 2, "wset_reserve", _merge(_ask(("train_windows",), lambda s: s.nf * s.sL * 4),
                                                                 _ask(("train_mix", "cv_mix", "mix_features"), lambda s: s.n * s.sL * 4)))),
    ("wset.r[2]", Buffer("r", "grow", 2, "wset_reserve", _ask(_WSET, lambda s: s.n_nat * D * 4))),
    ("wset.r[3]", Buffer("r", "grow", 2, "wset_reserve", _ask(_WSET, lambda s: 3 * s.n * 4))),
    ("out_chunk", Buffer("out_chunk", "frames", 1, "out_chunk_reserve", _ask(_FWD, _out_frames))),
    ("host_out", Buffer("host_out", "frames", 1, "out_chunk_reserve", _ask(_FWD, _out_frames))),
    ("wave[0]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _wave_in_bytes))),
    ("wave[1]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), lambda s: s.n * D * 8))),
    ("wave[2]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), lambda s: s.n * 2 * HOP * 4))),
    ("wave[3]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _pcm))),
    ("wave_pin[0]", Buffer("wave_pin", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _wave_in_bytes))),
    ("wave_pin[1]", Buffer("wave_pin", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _pcm))),
    ("in_d", Buffer("in_d", "grow", 1, "wave_grow:generate", _ask(MIXED, _mix_in_bytes))),
    ("x", Buffer("x", "grow", 1, "wave_grow:generate", _ask(MIXED, _pcm))),
    ("s", Buffer("s", "grow", 1, "wave_grow:generate", _ask(MIXED, _pcm))),
    ("v", Buffer("v", "grow", 1, "wave_grow:generate", _ask(MIXED, _pcm))),
    ("gain", Buffer("gain", "grow", 1, "wave_grow:generate", _ask(MIXED, lambda s: s.n_sent * 4))),
    ("lps", Buffer("lps", "grow", 1, "wave_grow:generate", _ask(("mix_features", "eval_mix"), lambda s: s.n * D * 4))),
    ("in_pin", Buffer("in_pin", "grow", 2, "wave_grow:generate", _ask(MIXED, _mix_in_bytes))),
    ("ev_Y", Buffer("ev_Y", "grow", 1, "wave_grow:eval", _ask(("eval_mix",), lambda s: s.n * D * 8))),
    ("ev_syn", Buffer("ev_syn", "grow", 1, "wave_grow:eval", _ask(("eval_mix",), lambda s: s.n * 2 * HOP * 4))),
    ("ev_ola", Buffer("ev_ola", "grow", 1, "wave_grow:eval", _ask(("eval_mix",), _pcm))),
    ("ev_lps", Buffer("ev_lps", "grow", 1, "wave_grow:eval", _ask(("eval_mix",), lambda s: 2 * al256(s.n * D * 4)))),
])
# Buffers of bp_eval_mix whose size follows the scoring plan (eval_plan: resampled lengths, STOI frames and segments per sentence),
# which this model does not restate: they are on record as buffers of the eval_mix kind, the walks run them at every size, and the
# regrow claim is not made for them.  ev_gain is asked for 0 bytes by every net-scored call (bp_eval_mix_logmmse alone sizes it).
UNMODELLED = collections.OrderedDict([
    ("ev_tab", "the table block of eval_plan plus the scores"), ("ev_work", "the work block of eval_plan"),
    ("ev_pin", "the pinned table block of eval_plan"), ("ev_gain", "0 bytes in bp_eval_mix (the log-MMSE gains of bp_eval_mix_logmmse)"),
])
# Every other Buf the sources declare, and why it is no state that a call's size leaves behind on a handle.
OTHER_BUFS = collections.OrderedDict([
    ("q", "dev_alloc's local, moved into allocs"), ("allocs", "the dev_alloc list itself (its sized blocks: the two fixed rows above)"),
    ("corpus", "allocated exactly by bp_set_mix_corpus"), ("reverb", "allocated exactly by bp_set_mix_reverb"),
    ("nb", "local to bp_set_mix_reverb"), ("hb", "local to bp_set_mix_reverb"),
    ("d", "the one block of a handle-less call (OneShot), freed on return"),
    ("dev", "a stream's block, allocated exactly when it opens"), ("pin_in", "a stream's block, allocated exactly when it opens"),
    ("pin_out", "a stream's block, allocated exactly when it opens"),
    ("sink_b", "local to bp_measure_peaks"), ("src_b", "local to bp_measure_peaks"), ("dst_b", "local to bp_measure_peaks"),
    ("sw", "local to bp_time_kernel"), ("sd", "local to bp_time_kernel"), ("sb", "local to bp_time_kernel"),
    ("dm_b", "local to bp_train_resident_masked, released on return"), ("xm_b", "local to bp_train_resident_masked, released on return"),
])
# The call sites the table was written from: (file, callee) -> how many calls the file holds (definitions and declarations apart).
SITES = {("bp_step.hip", "wset_reserve"): 2, ("bp_step.hip", "out_chunk_reserve"): 1, ("bp_mix.hip", "out_chunk_reserve"): 2,
         ("bp_wave.hip", "out_chunk_reserve"): 1, ("bp_stream.hip", "out_chunk_reserve"): 2, ("bp_mix.hip", "wave_grow"): 3,
         ("bp_wave.hip", "wave_grow"): 1}
# Which paths stage a bunch through the two tiles (stage_cur, pre.tile), so that the tile a training call starts in follows the
# bunches staged before it: window chunks always; stacked chunks when the visible dropout is on (presets with dropoutflag 1).
STAGING = "window chunks always, stacked chunks when visible dropout is on"


def asks(cfg, name, s):
    """What call s asks buffer `name` for (0: it does not touch it)."""
    fn = BUFFERS[name].ask.get(s.kind)
    if fn is None or (not s.ok and not (s.open_frames and BUFFERS[name].policy == "frames")):
        return 0
    return int(fn(_WithSL(s, sl_of(cfg))))


class _WithSL(object):
    def __init__(self, s, sL):
        self.__dict__.update(s._asdict(), sL=sL)


def sizing_kinds(name):
    return list(BUFFERS[name].ask)


def never_regrows(cfg, name):
    """True where the policy lets NO order of this model's calls regrow the buffer: its largest request fits what its smallest
    request allocates."""
    b = BUFFERS[name]
    if b.policy == "fixed":
        return True
    req = [asks(cfg, name, shape(cfg, k, z, 3 if z == "L" else None)) for k in b.ask for z in sizes_of(k) if z != "OVER"]
    nb_max = (CAP - (N_SHORT + 1) * (CTX - 1) - cfg.B // 2) // cfg.B             # (L with the most bunches the capacity holds)
    req_l = [asks(cfg, name, shape(cfg, k, "L", nb_max - 1 + nb_max % 2)) for k in b.ask]
    pos = [r for r in req if r > 0]
    return max(req + req_l) <= POLICY[b.policy](min(pos))


NEVER = ("stacked pair", "stage tiles", "in_d", "gain", "in_pin")  # by name; test_size_coverage holds it to never_regrows()

# (kind, buffer) pairs that L does NOT regrow behind M although the buffer can regrow, and why; by name, held by the coverage test
L_EXEMPT = {("stream", "wset.r[2]"): "a stream asks for n_chan nat rows: four channels are 528 bytes, a regrow behind M takes 34"}
_LARGE = {}


def large(cfg, kind):
    """The bunch count of L: the smallest odd nb >= 3 at which every buffer that `kind` sizes (NEVER apart) asks for more than an M
    call of the kind left it with."""
    key = (cfg.id, kind)
    if key not in _LARGE:
        m = shape(cfg, kind, "M")
        nb = 3
        while True:
            l = shape(cfg, kind, "L", nb)
            if l.rows <= CAP and kind in SENTENCES and kind != "stream" and l.T[0] < 2:
                nb += 2
                continue
            if all(asks(cfg, n, l) > POLICY[b.policy](asks(cfg, n, m)) for n, b in BUFFERS.items()
                   if kind in b.ask and n not in NEVER and (kind, n) not in L_EXEMPT and asks(cfg, n, m) > 0):
                break
            nb += 2
            assert nb * cfg.B < CAP, (cfg.id, kind, "no L under the capacity")
        assert l.rows < CAP
        _LARGE[key] = nb
    return _LARGE[key]


def families():
    """The families of kinds that share state: the maximal sets among the buffers' sizing kinds (a buffer whose kinds lie inside
    another's -- the mixing, evaluation and signal-layer buffers inside the staging sets' -- adds no pair).  name -> kinds."""
    sets = collections.OrderedDict()
    for name, b in BUFFERS.items():
        ks = tuple(k for k in SM.KINDS if k in b.ask)
        if ks not in sets.values():
            sets[name] = ks
    return collections.OrderedDict((n, ks) for n, ks in sets.items() if not any(set(ks) < set(o) for o in sets.values()))


FAMILY_IDS = collections.OrderedDict([("stacked pair", "stacked"), ("wset.r[0]", "wset"), ("out_chunk", "out")])


def family_of(fid):
    return families()[[n for n, i in FAMILY_IDS.items() if i == fid][0]]


# ------------------------------------------------------------------ the model
Step = collections.namedtuple("Step", "pos kind size status before after")
_PROBE = {}


def _leaves(kind):
    """(window chunk?, targets?) of what a sized kind leaves resident: sequence_model's own update, asked once."""
    if kind not in _PROBE:
        st = SM.fresh_state()
        SM.KINDS[kind].apply(SM.CONFIGS[0], st, 0)
        _PROBE[kind] = (st["windows"], st["has_targ"])
    return _PROBE[kind]


def run_model(cfg, calls, st=None):
    """The model over calls = [(pos, kind, size), ...] from a fresh handle."""
    st = SM.fresh_state() if st is None else dict(st)
    out = []
    for pos, kind, size in calls:
        k = SM.KINDS[kind]
        before = dict(st)
        if kind in SIZED:
            s = shape(cfg, kind, size)
            status = SM.BP_OK if s.ok else SM.BP_ERR_ARG
            if s.ok:
                w, t = _leaves(kind)
                SM._resident(st, pos, kind, s.resident, w, t)
                st["bunches"] += s.bunches
        else:
            why = k.pre(cfg, st)
            status = SM.BP_OK if why is None else k.fail[why]
            if why is None:
                k.apply(cfg, st, pos)
        out.append(Step(pos, kind, size, status, before, dict(st)))
    return out


def idle(cfg, step):
    """A successful training call that trains nothing (size Z)."""
    return step.kind in SIZED and SM.KINDS[step.kind].training and step.status == SM.BP_OK and shape(cfg, step.kind, step.size).bunches == 0


# ------------------------------------------------------------------ the walks
def nodes(cfg, kinds, over=False):
    return [(k, z) for k in kinds for z in sizes_of(k) if over or z != "OVER"]


def closed_walk(cfg, fid):
    """One closed walk that takes every ordered pair of the family's (kind, size) nodes once (sequence_model.closed_walk's
    construction on the nodes)."""
    ns = nodes(cfg, family_of(fid))
    K = len(ns)
    rng = np.random.default_rng([cfg.index, 11, list(FAMILY_IDS.values()).index(fid)])
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
    return [ns[i] for i in circuit]


# Pieces per family's closed walk, each a GPU test of its own from fresh handles (the rule of sequence_model.pieces: a piece starts
# with the call the one before it ended with).  Chosen from the measured times: every piece under ten seconds.
N_PIECES = collections.OrderedDict([("stacked", 4), ("wset", 8), ("out", 6)])
N_RANDOM, RANDOM_LEN = 4, 60


def pieces(cfg, fid, n_pieces=None):
    P = N_PIECES[fid] if n_pieces is None else n_pieces
    w = closed_walk(cfg, fid)
    n = len(w) - 1
    cuts = [round(i * n / P) for i in range(P + 1)]
    return [[(p,) + w[p] for p in range(cuts[i], cuts[i + 1] + 1)] for i in range(P)]


def over_walk(cfg):
    """OVER once behind every other size of its kind; the call behind an OVER is the next size's."""
    out = []
    for k in SIZED:
        for z in sizes_of(k):
            if z != "OVER":
                out += [(k, z), (k, "OVER")]
    out.append(("checkpoint", None))
    return [(p,) + n for p, n in enumerate(out)]


def random_walk(cfg, seed):
    """A kind of the configuration at random, then one of its sizes (OVER among them)."""
    ks = SM.kinds_of(cfg)
    rng = np.random.default_rng([cfg.index, 2000 + seed])
    out = []
    for p in range(RANDOM_LEN):
        k = ks[int(rng.integers(len(ks)))]
        zs = sizes_of(k)
        out.append((p, k, zs[int(rng.integers(len(zs)))]))
    return out


def walk_ids(cfg):
    return ["%s%d" % (f, i) for f, P in N_PIECES.items() for i in range(P)] + ["over"] + ["random%d" % s for s in range(N_RANDOM)]


def walk_calls(cfg, wid):
    """(walk number for the data, calls) of one walk id."""
    for j, (f, P) in enumerate(N_PIECES.items()):
        if wid.startswith(f) and wid[len(f):].isdigit():
            return j, pieces(cfg, f)[int(wid[len(f):])]
    if wid == "over":
        return len(N_PIECES), over_walk(cfg)
    s = int(wid[len("random"):])
    return len(N_PIECES) + 1 + s, random_walk(cfg, s)


def test_id(cfg, wid):
    return "tests/test_size_gpu.py::test_size_walk[%s-%s]" % (cfg.id, wid)


GPU_TESTS = [test_id(c, w) for c in SM.CONFIGS for w in walk_ids(c)]


def pair_table(cfg, fid, n_pieces=None):
    """((kind, size), (next kind, next size)) -> the GPU tests that run it."""
    out = {}
    for i, p in enumerate(pieces(cfg, fid, n_pieces)):
        for a, b in zip(p, p[1:]):
            out.setdefault((a[1:], b[1:]), []).append(test_id(cfg, "%s%d" % (fid, i)))
    return out


def all_walks(cfg):
    return [(wid,) + walk_calls(cfg, wid) for wid in walk_ids(cfg)]


# ------------------------------------------------------------------ what the policy does along a walk
def simulate(cfg, calls):
    """Along one walk from a fresh handle: per buffer the regrows (a growth of a block that exists: synchronise, free, unzeroed
    memory) and the kinds that ran a SMALLER request behind a regrow in the block it left."""
    cap = {n: [0] * b.slots for n, b in BUFFERS.items()}
    cur = {n: 0 for n in BUFFERS}
    regrows = collections.Counter()
    smaller = collections.defaultdict(set)
    regrown = {n: [False] * b.slots for n, b in BUFFERS.items()}
    for step in run_model(cfg, calls):
        if step.kind not in SIZED:
            continue
        s = shape(cfg, step.kind, step.size)
        for n, b in BUFFERS.items():
            a = asks(cfg, n, s)
            if a == 0 or b.policy == "fixed":
                continue
            for _ in range(max(s.uses, 1) if b.slots == 2 else 1):
                if b.slots == 2:
                    cur[n] ^= 1
                k = cur[n]
                if a > cap[n][k]:
                    if cap[n][k]:
                        regrows[n] += 1
                        regrown[n][k] = True
                    cap[n][k] = POLICY[b.policy](a)
                elif regrown[n][k] and POLICY[b.policy](a) < cap[n][k]:
                    smaller[n].add(step.kind)
    return regrows, smaller


# ------------------------------------------------------------------ data
_CORPUS = {}


def corpus_T(cfg):
    """(T, dyed) of every clean entry behind sequence_model's four."""
    need = []
    for k in MIXED:
        for z in GOOD + ("OVER",):
            if z == "M":
                continue
            dyed = z in DYED and not SM.KINDS[k].training
            for i, T in enumerate(shape(cfg, k, z).T):
                e = (T, dyed and not (k == "mix_features" and i == 0))
                if e not in need:
                    need.append(e)
    return need


def corpus(cfg):
    """sequence_model's recordings (the same lengths, so M is M), then one entry per (frames, dyed) that a size needs."""
    if cfg.id not in _CORPUS:
        rng = np.random.default_rng([cfg.index, 98])
        clean = [(rng.normal(size=n) * 3000.0).astype(np.float32) for n in SM.CLEAN_LEN]
        noise = [(rng.normal(size=n) * 1500.0).astype(np.float32) for n in SM.NOISE_LEN]
        mean = rng.normal(10.0, 2.0, D).astype(np.float32)
        inv_std = rng.uniform(0.2, 0.5, D).astype(np.float32)
        index = {}
        for T, dyed in corpus_T(cfg):
            index[(T, dyed)] = len(clean)
            x = (rng.normal(size=len_of(T)) * 3000.0).astype(np.float32)
            clean.append(np.full_like(x, np.nan) if dyed else x)
        _CORPUS[cfg.id] = dict(clean=clean, noise=noise, mean=mean, inv_std=inv_std, index=index)
    return _CORPUS[cfg.id]


def _plan(cfg, rng, kind, size, s):
    if size == "M":
        return SM._plan(rng, SM.train_clean(cfg) if kind == "train_mix" else SM.QUERY_CLEAN)
    idx = corpus(cfg)["index"]
    dyed = size in DYED and not SM.KINDS[kind].training
    return SM._plan(rng, [idx[(T, dyed and not (kind == "mix_features" and i == 0))] for i, T in enumerate(s.T)])


def dyed(kind, size):
    return size in DYED and kind in SIZED and not SM.KINDS[kind].training


def call_data(cfg, walk, pos, kind, size):
    """What the call at position pos of walk number `walk` is made with."""
    if kind not in SIZED:
        return {}
    rng = np.random.default_rng([cfg.index, 100 + walk, pos])
    s = shape(cfg, kind, size)
    nan = dyed(kind, size)
    if kind in STACKED:
        d = SM._stacked(cfg, rng, s.n)
        if kind == "grads":
            d["first"] = min(3, s.n - cfg.B)
        if nan:
            d["x"][cfg.B + 3 if kind == "grads" else 0:] = np.nan
        return d
    if kind in WINDOWS:
        d = SM._windows(cfg, rng, s.n)
        if s.n_nat != 2:
            d["nat"] = rng.normal(size=(s.n_nat, D)).astype(np.float32)
            d["nat_row"] = rng.integers(0, s.n_nat, s.n).astype(np.int32)
        if nan:
            d["fea"][:] = np.nan
            d["nat"][:] = np.nan
        return d
    if kind == "train_mix":
        return dict(plan=_plan(cfg, rng, kind, size, s), order=MX.shuffle(1 + pos, 10 * walk + cfg.index, s.n) if s.ok else np.arange(s.n))
    if kind in MIXED:
        return dict(plan=_plan(cfg, rng, kind, size, s))
    if kind == "enhance":
        lens = SM.ENHANCE_LEN if size == "M" else [len_of(T) for T in s.T]
        return dict(sentences=[np.full(n, np.nan, np.float32) if nan else (rng.normal(size=n) * 3000.0).astype(np.float32) for n in lens])
    nc, max_push, pushes, ends = s.pushes                        # stream
    blocks = [[np.full(n, np.nan, np.float32) if nan else (rng.normal(size=n) * 3000.0).astype(np.float32) for n in blk] for blk in pushes]
    return dict(blocks=blocks, ends=ends, max_push=max_push)


# ------------------------------------------------------------------ the figures of a GPU run
def numbers(parity):
    keep = {k: v for k, v in sorted(parity["tests"].items()) if "test_size_gpu.py" in k}
    return {"source": "a -m gpu run of tests/test_size_gpu.py on an MI355X; `python tests/size_model.py numbers <parity JSON> <out>` behind it",
            "bar": "bit for bit: words_differing == 0 in every entry", "tests": keep}


if __name__ == "__main__":
    import json
    import sys
    if len(sys.argv) == 4 and sys.argv[1] == "numbers":
        json.dump(numbers(json.load(open(sys.argv[2]))), open(sys.argv[3], "w"), indent=1, sort_keys=True)
    else:
        for cfg in SM.CONFIGS:
            print(cfg.id, {k: large(cfg, k) for k in SIZED})
            for f in FAMILY_IDS.values():
                print(" ", f, len(closed_walk(cfg, f)) - 1, "pairs")
