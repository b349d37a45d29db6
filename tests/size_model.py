"""The size layer of tests/sequence_model.py: the same handle, the same call kinds, calls of CHANGING size, and the two families of walks
that run them -- SIZE over the 19 kinds and three configurations of sequence_model.WALK, XSIZE over the whole table and configuration D.
Imports neither the package nor a GPU; tests/test_size_coverage.py and tests/test_xsize_coverage.py check everything in here on any
machine, tests/test_size_gpu.py and tests/test_xsize_gpu.py run the walks.

What sizes reach and constant sizes never do: the grow-only buffers of a handle (Buf::grow, csrc/bp_mem.h) are regrown -- the
streams named at the call site are synchronised, the old block is freed, n + n/4 + 4096 bytes of UNZEROED memory come back -- and a
small call runs in buffers whose tails hold a larger call's data.  BUFFERS below is the one table of those buffers, written from the
call sites (SITES): which kinds size a buffer and how many bytes a call asks for, as a function of the call's shape and the
noise-aware mode.  The families of kinds that share state, the size class L ("large enough that every buffer is regrown behind an M
call") and the regrow / shrink claims of the coverage tests are all computed from that table and the policy; nothing of it needs a
device.  A text scan (scan / scan_problems) holds the table to the sources: a Buf without a row, a fifth nat_b expression or a new
window_reserve site fails by name.

Size classes of a call (SIZES), rows per call with FEA_DIM 33, the configurations and bunch sizes of sequence_model, CAP 1024:
  Z     fewer rows than a bunch: one row (stacked and window kinds), one sentence of one sample (mix, enhance, eval, stream kinds).
        A training call of size Z trains nothing.
  ONE   exactly B rows: one bunch, an odd count
  M     the size of sequence_model's unsized walks: two bunches and a part (training), B + 3 rows or 41 frames (queries)
  L     nb bunches and half a bunch, nb the smallest odd count >= 3 at which every buffer the kind sizes, and that the policy lets
        regrow at all, is regrown behind an M call of that kind (large()); the sentence kinds take more sentences AND one long one
  FULL  exactly CAP rows
  OVER  CAP + 1 rows: BP_ERR_ARG, the model state stays as it was
The gradient query has no Z: its gradient is that of one whole bunch (NO_Z).  gv_mix and eval_mix_logmmse have the six classes and the
sentence shapes of eval_mix (the same frames per sentence, so the same corpus entries).  time_kernel and profile_step stay unsized:
their precondition reads the rows of whatever chunk is resident.

The table in the two families.  XSIZE reads BUFFERS whole.  SIZE reads it restricted to its kinds and in static mode (view), which is
the table as it stood before the noise-aware mode and the two new sized kinds: a static ask for the noise-aware rows is n_nat rows
whatever the site, and the asks for 0 bytes that a call site spells out (ZERO: bp_gv_mix on ev_syn, ev_ola and lps, the net-scored
calls on ev_gain -- such a kind does not size the buffer and leaves its block as it was) all belong to kinds or rows outside it.  The
one place where the view is no restriction has a name: LEGACY_UNMODELLED.
ev_tab, ev_work and ev_pin stay in UNMODELLED: tab_layout / work_walk of csrc/bp_eval.hip lay out some thirty tables per plan
(resampled lengths, STOI frames and segments, the LPC frame blocks of width 7), which is not short.  The claim made in their place
needs no byte count (width_pairs): in every configuration a scoring call of each width 3 / 5 / 7 at Z or ONE runs directly behind a
dyed L or FULL scoring call of each other width.

Dye: the query kinds at L and FULL carry NaN in their input (rows, PCM samples, the nat rows of window chunks), so every buffer they
touch is full of NaN when the next, smaller call runs, and a leak of remains shows as NaN, not as a small error.  Training kinds
stay finite.  The two queries that leave a chunk WITH targets (sequence_model.LOADABLE) keep the rows that a train_resident or
grads_resident behind them reads finite -- the first B + 3 rows of the gradient upload, the first mixture of mix_features -- so that
the net stays finite; everything behind those rows is NaN.  No entry point refuses non-finite samples or rows by design (only SNRs,
lc_db and impulse-response taps are checked), so FINITE_DYE, the kinds dyed with 3e38-scale values instead, is empty.
Read for the newer kinds, in csrc/: bp_eval_lpc (bp_eval.hip) loops over a.win, EV_FB and the template order P alone, and a frame of
NaN is INVALID by `pos = R[0] > 0.0` / `valid = pos && Rr[0] > 0.0` (NaN > 0 is false), so it is written as 0.0 with lv = 0;
bp_eval_lpcrank reads an invalid frame as +inf, its loop bounds come from the host's SJ table, every thread counts in ascending order
into its own integers, and no NaN is ever compared; bp_eval_lpcsum is a fixed tree; bp_wave_gv_parts (wave_gv_launch, bp_wave.hip) is
one thread per bin, serial over its part's frames in ascending order; lm_track (bp_classic.h) has "no decision in here: min, max and
the clamp only", lm_e1's two loops end at 64 and 200 whatever the comparison inside says, bp_wave_dnat loops over T from the host's F
table.  No data-dependent bound, no result that depends on the order of arrival: the output under NaN is a function of the input."""
import collections
import re
import sys

import numpy as np

import mix_np as MX
import sequence_model as SM
import stream_np as ST

CAP = 1024
SIZES = ("Z", "ONE", "M", "L", "FULL", "OVER")
GOOD = SIZES[:-1]
D, HOP, CTX = SM.FEA_DIM, SM.HOP, SM.CONTEXT
STATIC, DYNAMIC = 0, 1
STACKED = ("train", "upload_train", "forward", "cv", "grads")
WINDOWS = ("train_windows", "cv_windows")
NEW_SIZED = ("gv_mix", "eval_mix_logmmse")                     # sized like eval_mix
MIXED = ("train_mix", "cv_mix", "mix_features", "eval_mix") + NEW_SIZED      # generate()
SENTENCES = MIXED + ("enhance", "stream")
EVAL = ("eval_mix",) + NEW_SIZED                               # eval_mix_run
SCORED = ("eval_mix", "eval_mix_logmmse")                      # the kinds with a score width
KEEPS_Y = EVAL                                                 # generate() with a spectrum of the caller's (ev_Y)
NO_Y = ("train_mix", "cv_mix", "mix_features")                 # generate() without: in dynamic mode Y lies behind the nat rows
# the kinds whose nat_b follows the mode: sequence_model.READS_NAT, and bp_eval_mix_logmmse, which goes through generate() too
# (its scores do not read the rows; the tracker still writes them, one per frame)
ASKS_NAT = SM.READS_NAT + ("eval_mix_logmmse",)
NO_Z = {"grads": "the gradient is that of one whole bunch: a chunk of fewer rows has none"}
SIZES_OF = collections.OrderedDict((k, [s for s in SIZES if not (s == "Z" and k in NO_Z)]) for k in SM.KINDS if k in STACKED + WINDOWS + SENTENCES)
DYED = ("L", "FULL")
FINITE_DYE = ()                                                # kinds whose entry point refuses non-finite input by design: none
N_SHORT, SHORT_T = 34, 5                                       # L of the sentence kinds: 34 sentences of 5 frames and one long one
N_NAT_L = 40                                                   # nat rows of a window chunk at L and FULL (M: 2)
STREAM_L = dict(n_chan=4, max_push=16384, per_block=4000, pushes=2)


def sizes_of(kind):
    return SIZES_OF.get(kind, [None])


def sl_of(cfg):
    return cfg.ls[-1]


def len_of(T):
    """Samples of a sentence of T frames (T = (n - 1) // HOP + 2); T = 2: ONE sample."""
    return 1 if T == 2 else (T - 2) * HOP + 7


def dyed(kind, size):
    return size in DYED and not SM.KINDS[kind].training


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
    if kind in NEW_SIZED:
        return shape(cfg, "eval_mix", size, nb)._replace(kind=kind)
    if kind not in SIZES_OF:
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
# ask: {kind: view of a Shape -> bytes (frames for "frames") the call asks for}; the view adds sL, the net's output width, and dyn, the
# noise-aware mode; a kind that asks for 0 bytes does not size the buffer)
Buffer = collections.namedtuple("Buffer", "member policy slots site ask")


def _ask(kinds, fn):
    return collections.OrderedDict((k, fn) for k in kinds)


def _merge(*parts):
    out = collections.OrderedDict()
    for p in parts:
        out.update(p)
    return out


def ZERO(s):
    """An ask for 0 bytes that the call site spells out (wave_grow leaves the block as it is)."""
    return 0


def _mix_in_bytes(s):
    """Call::bytes of plan_call (csrc/bp_mix.hip): F | Fs | clean | noise | offset | snr | order."""
    m = s.n_sent
    return 2 * al256((m + 1) * 4) + 2 * al256(m * 4) + al256(m * 8) + al256(m * 4) + al256(s.n * 4)


def _wave_in_bytes(s):
    """WaveIn::bytes (csrc/bp_wave.hip): F | mean | inv_std | window | twiddles | padded PCM."""
    return al256((s.n_sent + 1) * 4) + 2 * al256(D * 4) + al256(2 * HOP * 4) + al256((HOP + 1) * 8) + al256((s.n + s.n_sent) * HOP * 4)


# wset.r[2], the nat_b of the four call sites.  Per site: file -> the expression as it stands in the source (the text scan finds every
# `nat_b = ...;` of csrc/ and fails on one that is not here), and the ask in model terms, static and dynamic.
#   s.n frames (a stream: the frames due in its largest push), s.n_sent sentences / mixtures / channels, s.n_nat rows of an upload
NAT_EXPR = collections.OrderedDict([
    ("bp_step.hip", "nat ? (size_t)c->n_nat * D * 4 : 0"),
    ("bp_mix.hip", "!ms->nat ? 0 : !dyn ? (size_t)c.n * D * 4 : Y ? c.frames * D * 4 : dnat_b + c.frames * D * sizeof(float2)"),
    ("bp_wave.hip", "!nat ? 0 : dyn ? p.frames * D * 4 : (size_t)c->n_sent * D * 4"),
    ("bp_stream.hip", "!s->nat ? 0 : s->dyn ? (size_t)n * D * 4 : (size_t)nc * D * 4"),
])
DNAT_B = "const size_t dnat_b = al256(c.frames * D * 4);"     # bp_mix.hip: where the Y tail starts
WINDOW_RESERVE_SITES = {"bp_mix.hip": 1, "bp_wave.hip": 1, "bp_stream.hip": 1}


def y_tail(s):
    """Byte offset of the spectrum behind the nat rows of a dynamic call that keeps none (dnat_b)."""
    return al256(s.n * D * 4)


_per_sentence = lambda s: s.n_sent * D * 4
_per_frame = lambda s: s.n * D * 4
NAT_ASK = collections.OrderedDict(
    [(k, ("bp_step.hip", lambda s: s.n_nat * D * 4, lambda s: s.n_nat * D * 4)) for k in WINDOWS] +        # the caller's rows, either mode
    [(k, ("bp_mix.hip", _per_sentence, lambda s: y_tail(s) + s.n * D * 8)) for k in NO_Y] +
    [(k, ("bp_mix.hip", _per_sentence, _per_frame)) for k in KEEPS_Y] +
    [("enhance", ("bp_wave.hip", _per_sentence, _per_frame)), ("stream", ("bp_stream.hip", _per_sentence, _per_frame))])


def _nat_ask(s):
    return NAT_ASK[s.kind][2 if s.dyn else 1](s)


def _static_nat_ask(s):
    """The static ask whatever the mode: the row before the mode was part of it (the mutant of the coverage test)."""
    return s.n_nat * D * 4


_pcm = lambda s: (s.n + s.n_sent) * HOP * 4                   # segs * hop * 4: a sentence of T frames takes T + 1 segments
_rows_f32 = lambda s: s.n * D * 4
_syn = lambda s: s.n * 2 * HOP * 4
_WSET = WINDOWS + SENTENCES
# (`if (!lm ...) out_chunk_reserve`: the log-MMSE call runs no net)
_FWD = ("forward", "cv", "cv_windows", "cv_mix", "enhance", "eval_mix", "stream", "gv_mix")
_out_frames = lambda s: max(s.n if s.ok else 0, s.open_frames)
_GV_ZERO = _ask(("gv_mix",), ZERO)

BUFFERS = collections.OrderedDict([
    ("stacked pair", Buffer("allocs", "fixed", 2, "dev_alloc", _ask(STACKED, lambda s: s.n))),
    # (the window kinds stage through the tiles too: every pair of them is in the staging sets' family)
    ("stage tiles", Buffer("allocs", "fixed", 2, "dev_alloc", _ask(("train", "upload_train", "grads"), lambda s: s.n))),
    ("wset.r[0]", Buffer("r", "grow", 2, "wset_reserve", _merge(_ask(WINDOWS, lambda s: s.nf * D * 4), _ask(SENTENCES, lambda s: s.rows * D * 4)))),
    ("wset.r[1]", Buffer("r", "grow", 2, "wset_reserve", _merge(_ask(("train_windows",), lambda s: s.nf * s.sL * 4),
                                                                 _ask(("train_mix", "cv_mix", "mix_features"), lambda s: s.n * s.sL * 4)))),
    ("wset.r[2]", Buffer("r", "grow", 2, "wset_reserve", _ask(list(NAT_ASK), _nat_ask))),
    ("wset.r[3]", Buffer("r", "grow", 2, "wset_reserve", _ask(_WSET, lambda s: 3 * s.n * 4))),
    ("out_chunk", Buffer("out_chunk", "frames", 1, "out_chunk_reserve", _ask(_FWD, _out_frames))),
    ("host_out", Buffer("host_out", "frames", 1, "out_chunk_reserve", _ask(_FWD, _out_frames))),
    ("wave[0]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _wave_in_bytes))),
    ("wave[1]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), lambda s: s.n * D * 8))),
    ("wave[2]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _syn))),
    ("wave[3]", Buffer("wave", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _pcm))),
    ("wave_pin[0]", Buffer("wave_pin", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _wave_in_bytes))),
    ("wave_pin[1]", Buffer("wave_pin", "grow", 1, "wave_grow:enhance", _ask(("enhance",), _pcm))),
    ("in_d", Buffer("in_d", "grow", 1, "wave_grow:generate", _ask(MIXED, _mix_in_bytes))),
    ("x", Buffer("x", "grow", 1, "wave_grow:generate", _ask(MIXED, _pcm))),
    ("s", Buffer("s", "grow", 1, "wave_grow:generate", _ask(MIXED, _pcm))),
    ("v", Buffer("v", "grow", 1, "wave_grow:generate", _ask(MIXED, _pcm))),
    ("gain", Buffer("gain", "grow", 1, "wave_grow:generate", _ask(MIXED, lambda s: s.n_sent * 4))),
    ("lps", Buffer("lps", "grow", 1, "wave_grow:generate", _merge(_ask(("mix_features",) + SCORED, _rows_f32), _GV_ZERO))),
    ("in_pin", Buffer("in_pin", "grow", 2, "wave_grow:generate", _ask(MIXED, _mix_in_bytes))),
    ("ev_Y", Buffer("ev_Y", "grow", 1, "wave_grow:eval", _ask(EVAL, lambda s: s.n * D * 8))),
    ("ev_syn", Buffer("ev_syn", "grow", 1, "wave_grow:eval", _merge(_ask(SCORED, _syn), _GV_ZERO))),
    ("ev_ola", Buffer("ev_ola", "grow", 1, "wave_grow:eval", _merge(_ask(SCORED, _pcm), _GV_ZERO))),
    ("ev_lps", Buffer("ev_lps", "grow", 1, "wave_grow:eval", _merge(_ask(SCORED, lambda s: 2 * al256(s.n * D * 4)),
                                                                      _ask(("gv_mix",), lambda s: al256(s.n * D * 4))))),
    ("ev_gain", Buffer("ev_gain", "grow", 1, "wave_grow:eval", _merge(_ask(("eval_mix_logmmse",), lambda s: s.n * (D + 1) * 4),
                                                                        _ask(("eval_mix", "gv_mix"), ZERO)))),
])
# Buffers of the scoring calls whose size follows the scoring plan (eval_plan: resampled lengths, STOI frames and segments per
# sentence), which this model does not restate: they are on record as buffers of the eval kinds, the walks run them at every size, and
# the regrow claim is not made for them.
UNMODELLED = collections.OrderedDict([
    ("ev_tab", "the table block of eval_plan plus the scores"), ("ev_work", "the work block of eval_plan"),
    ("ev_pin", "the pinned table block of eval_plan"),
])
# Where the view of the 19 kinds is NOT the restriction of the table: ev_gain is asked for 0 bytes by every net-scored call
# (bp_eval_mix_logmmse alone sizes it), so no kind of the view sizes it and it is on record there as one of the unmodelled blocks.
LEGACY_UNMODELLED = collections.OrderedDict([("ev_gain", "0 bytes in bp_eval_mix (the log-MMSE gains of bp_eval_mix_logmmse)")])
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
# the buffers whose ask depends on the mode or on WHICH kind of a site makes the call (the coverage test makes its claims for these)
BY_MODE = ("wset.r[2]",)
BY_KIND = ("lps", "ev_syn", "ev_ola", "ev_lps", "ev_gain")


def unmodelled(fam):
    return UNMODELLED if "eval_mix_logmmse" in fam.kinds else collections.OrderedDict(list(UNMODELLED.items()) + list(LEGACY_UNMODELLED.items()))


def _restrict(kinds):
    rows = [(n, b._replace(ask=collections.OrderedDict((k, fn) for k, fn in b.ask.items() if k in kinds))) for n, b in BUFFERS.items()]
    return collections.OrderedDict((n, b) for n, b in rows if "eval_mix_logmmse" in kinds or n not in LEGACY_UNMODELLED)


def view(fam):
    """BUFFERS as the family sees it: every row's asks restricted to its kinds (SIZE: and ev_gain among the unmodelled blocks)."""
    return _restrict(fam.kinds)


class _View(object):
    def __init__(self, s, sL, dyn):
        self.__dict__.update(s._asdict(), sL=sL, dyn=dyn)


def asks(cfg, name, s, nat=STATIC, buffers=None):
    """What call s asks buffer `name` for in noise-aware mode `nat` (0: it does not size it)."""
    b = (buffers or BUFFERS)[name]
    fn = b.ask.get(s.kind)
    if fn is None or (not s.ok and not (s.open_frames and b.policy == "frames")):
        return 0
    return int(fn(_View(s, sl_of(cfg), bool(nat))))


def sizing_kinds(name, buffers=None):
    return [k for k, fn in (buffers or BUFFERS)[name].ask.items() if fn is not ZERO]


def zero_kinds(name, buffers=None):
    return [k for k, fn in (buffers or BUFFERS)[name].ask.items() if fn is ZERO]


def never_regrows(cfg, name, buffers=None):
    """True where the policy lets NO order of this model's calls regrow the buffer: its largest request fits what its smallest
    request allocates."""
    b = (buffers or BUFFERS)[name]
    if b.policy == "fixed":
        return True
    req = [asks(cfg, name, shape(cfg, k, z, 3 if z == "L" else None)) for k in b.ask for z in sizes_of(k) if z != "OVER"]
    nb_max = (CAP - (N_SHORT + 1) * (CTX - 1) - cfg.B // 2) // cfg.B             # (L with the most bunches the capacity holds)
    req_l = [asks(cfg, name, shape(cfg, k, "L", nb_max - 1 + nb_max % 2)) for k in b.ask]
    pos = [r for r in req if r > 0]
    return max(req + req_l) <= POLICY[b.policy](min(pos))


NEVER = ("stacked pair", "stage tiles", "in_d", "gain", "in_pin")  # by name; test_size_coverage holds it to never_regrows()

# (kind, buffer) pairs that L does NOT regrow behind M in static mode although the buffer can regrow, and why; by name, held by the
# coverage test
L_EXEMPT = {("stream", "wset.r[2]"): "a stream asks for n_chan nat rows: four channels are 528 bytes, a regrow behind M takes 34"}
# (kind, buffer, mode) cells among the newer ones -- the two new sized kinds, and every kind's dynamic ask -- likewise: none.  (In
# dynamic mode a stream asks for a row per frame due, 520 at L.)
L_EXEMPT_NEW = {}
_LARGE = {}


def large(cfg, kind):
    """The bunch count of L: the smallest odd nb >= 3 at which every buffer that `kind` sizes (NEVER apart) asks for more, in static
    mode, than an M call of the kind left it with."""
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
    """The families of the 19 kinds that share state: the maximal sets among the buffers' sizing kinds (a buffer whose kinds lie inside
    another's -- the mixing, evaluation and signal-layer buffers inside the staging sets' -- adds no pair).  name -> kinds."""
    sets = collections.OrderedDict()
    for name, b in _restrict(SM.WALK.kinds).items():
        ks = tuple(k for k in SM.KINDS if k in b.ask)
        if ks not in sets.values():
            sets[name] = ks
    return collections.OrderedDict((n, ks) for n, ks in sets.items() if not any(set(ks) < set(o) for o in sets.values()))


FAMILY_IDS = collections.OrderedDict([("stacked pair", "stacked"), ("wset.r[0]", "wset"), ("out_chunk", "out")])


def family_of(fid):
    return families()[[n for n, i in FAMILY_IDS.items() if i == fid][0]]


# ------------------------------------------------------------------ BUFFERS against the sources (a text scan)
def scan(texts):
    """What the sources hold, from {file name: text}: the Buf members, the members that wave_grow lists, the growing call sites per
    (file, callee), every nat_b expression per file and the window_reserve calls per file."""
    members, grown_args, sites, nat_b, reserve = set(), set(), collections.Counter(), collections.defaultdict(list), collections.Counter()
    for name, text in sorted(texts.items()):
        for m in re.finditer(r"\bBuf\s+([^;()=]+);", text):
            for v in m.group(1).split(","):
                v = v.strip()
                if v and v[0] not in "&*":
                    members.add(re.sub(r"\[.*", "", v))
        members.update(re.findall(r"vector<Buf>\s+(\w+)", text))
        for m in re.finditer(r"(?<![\w])(wave_grow|wset_reserve|out_chunk_reserve|window_reserve)\(([^;]*);", text):
            line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
            if re.search(r"\b(int|inline)\s*$", line):          # the definition or the declaration
                continue
            if m.group(1) == "window_reserve":
                reserve[name] += 1
                continue
            sites[(name, m.group(1))] += 1
            if m.group(1) == "wave_grow":
                grown_args.update(re.sub(r"\[.*", "", a) for a in re.findall(r"\{\s*(?:ms|h)->([\w\[\]]+)\s*,", m.group(2)))
        for m in re.finditer(r"\bsize_t\s+nat_b\s*=\s*([^;,]+)", text):
            nat_b[name].append(" ".join(m.group(1).split()))
    return dict(members=members, grown_args=grown_args, sites=dict(sites), nat_b=dict(nat_b), reserve=dict(reserve))


def scan_problems(found, buffers=None, unmodelled=None):
    """What is wrong between the sources and the table, each problem by name."""
    buffers = BUFFERS if buffers is None else buffers
    unmodelled = UNMODELLED if unmodelled is None else unmodelled
    known = set(b.member for b in buffers.values()) | set(unmodelled) | set(OTHER_BUFS)
    out = ["a Buf without a row: %s" % m for m in sorted(found["members"] - known)]
    out += ["a row for a Buf the sources no longer hold: %s" % m for m in sorted(known - found["members"])]
    table = set(b.member for b in buffers.values() if b.site.startswith("wave_grow")) | set(unmodelled)
    out += ["wave_grow sizes %s, which no row names" % m for m in sorted(found["grown_args"] - table)]
    out += ["a wave_grow row for %s, which no wave_grow call lists" % m for m in sorted(table - found["grown_args"])]
    if found["sites"] != SITES:
        out.append("the growing call sites are %r" % (sorted(found["sites"].items()),))
    for f, exprs in sorted(found["nat_b"].items()):
        out += ["a nat_b expression in %s that the wset.r[2] row does not restate: %s" % (f, e) for e in exprs if NAT_EXPR.get(f) != e]
    out += ["no nat_b expression left in %s" % f for f in NAT_EXPR if not found["nat_b"].get(f)]
    out += ["%s holds %d window_reserve calls, the table %d" % (f, found["reserve"].get(f, 0), WINDOW_RESERVE_SITES.get(f, 0))
            for f in sorted(set(found["reserve"]) | set(WINDOW_RESERVE_SITES)) if found["reserve"].get(f, 0) != WINDOW_RESERVE_SITES.get(f, 0)]
    used = set(f for f, _, _ in NAT_ASK.values())
    out += ["no kind of the wset.r[2] row is asked at the site in %s" % f for f in NAT_EXPR if f not in used]
    if "wset.r[2]" in buffers:
        out += ["%s sizes wset.r[0] and not wset.r[2]" % k for k in buffers["wset.r[0]"].ask if k not in buffers["wset.r[2]"].ask]
    return out


# ------------------------------------------------------------------ the walks by construction
def over_walk(cfg):
    """SIZE: OVER once behind every other size of its kind; the call behind an OVER is the next size's."""
    out = []
    for k, zs in SIZE.sizes.items():
        for z in zs:
            if z != "OVER":
                out += [(k, z), (k, "OVER")]
    out.append(("checkpoint", None))
    return [(p,) + n for p, n in enumerate(out)]


def _seq_calls(seq):
    return SM.with_modes([(i + 1,) + n for i, n in enumerate(seq)]) + [(2 * len(seq) + 2, "checkpoint", None)]


def mode_over_walk(cfg):
    """XSIZE: OVER once behind every other size of its kind: the two new sized kinds in static mode, then every kind whose
    noise-aware rows follow the mode in DYNAMIC mode."""
    seq = []
    for m, kinds in ((STATIC, NEW_SIZED), (DYNAMIC, ASKS_NAT)):
        for k in kinds:
            for z in sizes_of(k):
                if z != "OVER":
                    seq += [(k, z, m), (k, "OVER", m)]
    return _seq_calls(seq)


def full_walk(cfg):
    """ONE and FULL in dynamic mode, which the closed nat walk leaves out, by construction: per kind ONE and FULL in dynamic mode, Z
    in static mode behind it, FULL in static mode, Z in dynamic mode behind it."""
    seq = []
    for k in ASKS_NAT:
        seq += [(k, "ONE", DYNAMIC), (k, "FULL", DYNAMIC), (k, "Z", STATIC), (k, "FULL", STATIC), (k, "Z", DYNAMIC)]
    return _seq_calls(seq)


def regrow_walk(cfg):
    """What a seeded walk reaches by luck alone, by construction.
    1. The noise-aware rows regrown in STATIC mode behind a dynamic call.  A static ask is n_sent rows, a dynamic one a row per
       frame, so only the smallest dynamic call of a kind that keeps its spectrum elsewhere leaves a block that a static call
       outgrows (264 bytes grow to 4426, the 35 sentences of L ask for 4620): two dynamic Z calls, one per staging set, then two
       static L calls.
    2. ev_gain regrown by the log-MMSE call directly behind a net-scored call, three times (M, L, FULL), with gv_mix, which asks for
       none of it, behind both.
    3. The mask target under post-processing: bp_eval_mix at positions whose choice is the mask target, behind a set_post -- the
       header's BP_ERR_ARG with nothing touched on the nets with mask columns -- then one on the LPS target, which succeeds."""
    out = [(1, "set_nat", None), (2, "gv_mix", "Z"), (3, "enhance", "Z"), (4, "set_nat", None), (5, "eval_mix", "L"), (6, "enhance", "L")]
    seq = [("eval_mix_logmmse", "Z"), ("eval_mix", "M"), ("eval_mix_logmmse", "M"), ("gv_mix", "Z"), ("eval_mix", "L"), ("eval_mix_logmmse", "L"),
           ("eval_mix", "FULL"), ("eval_mix_logmmse", "FULL"), ("eval_mix", "Z"), ("gv_mix", "Z"), ("set_post", None)]
    out += [(7 + i,) + n for i, n in enumerate(seq)]
    p = out[-1][0]
    for masked, size in ((True, "Z"), (True, "L"), (False, "M"), (True, "ONE")):
        p = next(q for q in range(p + 1, p + 64) if SM.choice(cfg, q, "eval_mix")["masked"] == masked)
        out.append((p, "eval_mix", size))
    return out + [(p + 1, "gv_mix", "Z"), (p + 2, "checkpoint", None)]


_OUT_QUERIES = ("forward", "cv_windows", "enhance", "eval_mix", "stream")
MEASURE_SIZES = GOOD


def sized_measure_walk(cfg, size):
    """A stacked chunk of `size` in front of time_kernel, then every training kind, then a checkpoint; the same with profile_step
    behind a chunk with targets (a window chunk); and behind a time_kernel one query of the out_chunk family at L, so that the
    call after a timing run regrows what it may overwrite.  Kernel ids by position (sequence_model.choice)."""
    out = []
    for i, t in enumerate(SM.TRAINING_KINDS):
        tz = (t, "M" if t in SIZES_OF else None)
        out += [("train" if i % 2 == 0 else "upload_train", size), ("time_kernel", None), tz, ("checkpoint", None),
                ("train", size), ("time_kernel", None), (_OUT_QUERIES[i], "L"),
                ("train_windows", size), ("profile_step", None), tz, ("checkpoint", None)]
    return [(p,) + n for p, n in enumerate(out)]


# ------------------------------------------------------------------ the two families
# Pieces per closed walk, each a GPU test of its own from fresh handles (sequence_model.cut), chosen from measured seconds
# so that every piece stays under ten: SIZE's from its whole walks; XSIZE's from one run with 4 and 12 pieces (up to 17.2 s per whole
# ev walk and 62.8 s per whole nat walk, slowest piece 6.95 s), so that the slowest piece of that day stays a factor of two under.
EV_KINDS = ("eval_mix", "gv_mix", "eval_mix_logmmse", "mix_features")    # the kinds of the ev_* buffers and the fourth that sizes lps
NAT_KINDS = SM.READS_NAT
NAT_SIZES = ("Z", "M", "L")                                    # the closed nat walk (ONE and FULL: full_walk, the random walks)
EV_SEED = 40                                                   # the first seed at which width_pairs holds in all four configurations
LAYER = sys.modules[__name__]
SIZE = SM.WALK._replace(
    name="size", sizes=collections.OrderedDict((k, z) for k, z in SIZES_OF.items() if k in SM.WALK.kinds), layer=LAYER, cap=CAP,
    closed=[SM.Closed(f, pieces=P, walk=j, seed=(11, j), kinds=family_of(f), sizes=GOOD, modes=None)
            for j, (f, P) in enumerate([("stacked", 4), ("wset", 8), ("out", 6)])],
    built=[SM.Built("over", 3, over_walk)], random_seed=2000, random_no=4, corpus_seeds=(98, None),
    gpu_file="test_size_gpu.py", gpu_test="test_size_walk", timed=True)
# (the walk numbers lie behind those of the three other families)
XSIZE = SM.EXTENDED._replace(
    name="xsize", sizes=SIZES_OF, layer=LAYER, cap=CAP,
    closed=[SM.Closed("ev", pieces=6, walk=20, seed=(31, 0, EV_SEED), kinds=EV_KINDS, sizes=GOOD, modes=None),
            SM.Closed("nat", pieces=20, walk=21, seed=(31, 1, 0), kinds=NAT_KINDS, sizes=NAT_SIZES, modes=(STATIC, DYNAMIC))],
    built=[SM.Built("xover", 22, mode_over_walk), SM.Built("xfull", 23, full_walk), SM.Built("xregrow", 33, regrow_walk)] +
          [SM.Built("xmeasure%s" % z, 24 + i, lambda cfg, z=z: sized_measure_walk(cfg, z)) for i, z in enumerate(MEASURE_SIZES)],
    random_seed=4000, random_no=29, corpus_seeds=(99, 97), twins=True, gpu_file="test_xsize_gpu.py", gpu_test="test_xsize_walk")
FAMILIES = collections.OrderedDict((f.name, f) for f in (SM.WALK, SM.EXTENDED, SIZE, XSIZE))


def width_of(cfg, step):
    return SM.choice(cfg, step.pos, step.kind)["width"] if step.kind in SCORED else None


def width_pairs(cfg, calls):
    """(width of a dyed L or FULL scoring call, width of the scoring call at Z or ONE directly behind it), both successful."""
    steps = SM.run_model(XSIZE, cfg, calls)
    return set((width_of(cfg, a), width_of(cfg, b)) for a, b in zip(steps, steps[1:])
               if a.kind in SCORED and b.kind in SCORED and a.size in DYED and b.size in ("Z", "ONE") and a.status == b.status == SM.BP_OK)


WIDTH_PAIRS = set((a, b) for a in SM.WIDTHS for b in SM.WIDTHS if a != b)


def ev_seed_holds(seed):
    return all(set().union(*[width_pairs(c, p) for p in SM.pieces(XSIZE, c, "ev", salt=seed)]) >= WIDTH_PAIRS for c in XSIZE.configs)


# ------------------------------------------------------------------ what the policy does along a walk
Sim = collections.namedtuple("Sim", "regrows by_mode smaller by_prev zero_behind tail_moves behind_time")


def simulate(fam, cfg, calls, buffers=None):
    """Along one walk from a fresh handle, per buffer of the family's view:
    regrows      growths of a block that exists (synchronise, free, unzeroed memory)
    by_mode      ... of those that are owed to the mode -- the block was last sized in the OTHER mode, and in that mode this call
                 would have asked for another count of bytes: (mode of the block, mode of the call) -> count
    smaller      (kind, mode) that ran a SMALLER request behind a regrow in the block it left
    by_prev      (kind of the call directly before, kind that regrows the block) -> count
    zero_behind  (kind that asks for 0 bytes and leaves a REGROWN block alone, kind of the call directly before it)
    and over the walk: tail_moves, the NO_Y kinds whose Y tail starts at another byte offset than the dynamic NO_Y call directly
    before them; behind_time, the regrows of out_chunk by the call directly behind a successful time_kernel."""
    B = view(fam) if buffers is None else buffers
    cap = {n: [0] * b.slots for n, b in B.items()}
    cur = {n: 0 for n in B}
    last = {n: [None] * b.slots for n, b in B.items()}
    regrown = {n: [False] * b.slots for n, b in B.items()}
    regrows, by_mode, by_prev = collections.Counter(), collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    smaller, zero_behind = collections.defaultdict(set), collections.defaultdict(set)
    tail_moves, behind_time = set(), 0
    prev = None
    for step in SM.run_model(fam, cfg, calls):
        if step.kind not in fam.sizes:
            if step.kind != "set_nat":
                prev = step
            continue
        s, nat = shape(cfg, step.kind, step.size), step.before["nat"]
        if step.status == SM.BP_OK and nat == DYNAMIC and step.kind in NO_Y:
            if prev is not None and prev.kind in NO_Y and prev.status == SM.BP_OK and prev.before["nat"] == DYNAMIC \
                    and y_tail(shape(cfg, prev.kind, prev.size)) != y_tail(s):
                tail_moves.add(step.kind)
        for n, b in B.items():
            fn = b.ask.get(step.kind)
            if fn is ZERO and s.ok and step.status == SM.BP_OK:
                if regrown[n][0] and prev is not None:
                    zero_behind[n].add((step.kind, prev.kind))
                continue
            a = asks(cfg, n, s, nat, B) if step.status == SM.BP_OK or not s.ok else 0
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
                        if last[n][k][1] != nat and asks(cfg, n, s, 1 - nat, B) != a:
                            by_mode[n][(last[n][k][1], nat)] += 1
                        by_prev[n][(prev.kind if prev is not None else None, step.kind)] += 1
                        if n == "out_chunk" and prev is not None and prev.kind == "time_kernel" and prev.status == SM.BP_OK:
                            behind_time += 1
                    cap[n][k] = POLICY[b.policy](a)
                    last[n][k] = (step.kind, nat)
                elif regrown[n][k] and POLICY[b.policy](a) < cap[n][k]:
                    smaller[n].add((step.kind, nat))
        prev = step
    return Sim(regrows, by_mode, smaller, by_prev, zero_behind, tail_moves, behind_time)


# ------------------------------------------------------------------ data
_CORPUS = {}


def corpus_T(cfg):
    """(T, dyed) of every clean entry behind sequence_model's four."""
    need = []
    for k in MIXED:
        for z in GOOD + ("OVER",):
            if z == "M":
                continue
            dy = dyed(k, z)
            for i, T in enumerate(shape(cfg, k, z).T):
                e = (T, dy and not (k == "mix_features" and i == 0))
                if e not in need:
                    need.append(e)
    return need


def sized_corpus(fam, cfg):
    """sequence_model's recordings (the same lengths, so M is M; XSIZE: the very ones of EXTENDED), then one entry per (frames, dyed)
    that a size needs (index).  With fam.twins, on D every entry behind the first four also gets a reverberated twin, so that the
    derived entries appear in plans at every size: twin[i] is the corpus index of entry i's."""
    if (fam.name, cfg.id) not in _CORPUS:
        first, then = fam.corpus_seeds
        cor, rng = SM.recordings(cfg, first)
        if then is not None:
            rng = np.random.default_rng([cfg.index, then])
        clean, index = list(cor["clean"]), {}
        for T, dy in corpus_T(cfg):
            index[(T, dy)] = len(clean)
            x = (rng.normal(size=len_of(T)) * 3000.0).astype(np.float32)
            clean.append(np.full_like(x, np.nan) if dy else x)
        cor.update(clean=clean, index=index)
        if fam.twins:
            cor["twin"] = {}
            if SM.has_reverb(cfg):
                n0, n = len(SM.CLEAN_LEN), len(clean)
                extra = list(range(n0, n))
                cor["twin"] = dict([(c, n + j) for j, c in enumerate(cor["pair_clean"])] + [(c, n + len(SM.REVERB_PAIRS) + j) for j, c in enumerate(extra)])
                cor["pair_clean"] = list(cor["pair_clean"]) + extra
                cor["pair_rir"] = list(cor["pair_rir"]) + [i % len(cor["rirs"]) for i in range(len(extra))]
        _CORPUS[(fam.name, cfg.id)] = cor
    return _CORPUS[(fam.name, cfg.id)]


def source_of(fam, cfg, entry):
    """The clean entry a plan's index stands for (a derived entry: the sentence it was made from)."""
    cor = sized_corpus(fam, cfg)
    return entry if entry < len(cor["clean"]) else cor["pair_clean"][entry - len(cor["clean"])]


def frames_of_entry(fam, cfg, entry):
    return SM.frames_of(len(sized_corpus(fam, cfg)["clean"][source_of(fam, cfg, entry)]))


def _plan(fam, cfg, rng, kind, size, s):
    cor = sized_corpus(fam, cfg)
    if size == "M":                                            # sequence_model's plans: on D entries 4 and 5 are the derived ones
        clean = SM.plan_train_clean(cfg) if kind == "train_mix" else SM.plan_query_clean(cfg)
        n0 = len(SM.CLEAN_LEN)
        return SM.mixtures(rng, [c if c < n0 else len(cor["clean"]) + c - n0 for c in clean])
    dy = dyed(kind, size)
    clean = [cor["index"][(T, dy and not (kind == "mix_features" and i == 0))] for i, T in enumerate(s.T)]
    twin = cor.get("twin", {})
    return SM.mixtures(rng, [twin.get(c, c) if i % 2 == 0 else c for i, c in enumerate(clean)])


def sized_data(fam, cfg, walk, pos, kind, size):
    """The arrays and plans of a sized call (sequence_model.call_data puts what the call asks for beyond them in front)."""
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
    if kind in MIXED:
        d = dict(plan=_plan(fam, cfg, rng, kind, size, s))
        if kind == "train_mix":
            d["order"] = MX.shuffle(1 + pos, 10 * walk + cfg.index, s.n) if s.ok else np.arange(s.n)
        return d
    if kind == "enhance":
        lens = SM.ENHANCE_LEN if size == "M" else [len_of(T) for T in s.T]
        return dict(sentences=[np.full(n, np.nan, np.float32) if nan else (rng.normal(size=n) * 3000.0).astype(np.float32) for n in lens])
    nc, max_push, pushes, ends = s.pushes                        # stream
    blocks = [[np.full(n, np.nan, np.float32) if nan else (rng.normal(size=n) * 3000.0).astype(np.float32) for n in blk] for blk in pushes]
    return dict(blocks=blocks, ends=ends, max_push=max_push)
