"""The size axis of tests/size_model.py over the EXTENDED table of tests/sequence_model.py (XKINDS, configuration D): the two queries
that share the ev_* buffers with bp_eval_mix get sizes, the noise-aware mode becomes part of what a buffer is asked for, and the two
measurement calls run behind chunks of every size.  Imports neither the package nor a GPU; tests/test_xsize_coverage.py checks
everything in here on any machine, tests/test_xsize_gpu.py runs the walks.  size_model's kinds, sizes, walks, ids and data stay as
they are: this module only reads them.

Sized kinds: size_model.SIZED, then gv_mix and eval_mix_logmmse with the six size classes and the sentence shapes of eval_mix (the
same frames per sentence, so the same corpus entries).  time_kernel and profile_step stay unsized: their precondition reads the
rows of whatever chunk is resident.

BUFFERS here is size_model.BUFFERS with
  * the new kinds in every row whose call site they reach (generate(), eval_mix_run(): csrc/bp_mix.hip);
  * the noise-aware rows (wset.r[2]) as a function of the MODE: NAT_ASK restates the four nat_b expressions of the sources, which
    the text scan (scan / scan_problems) holds to the text, so a fifth expression or a new window_reserve site fails by name;
  * ev_gain out of UNMODELLED (bp_eval_mix_logmmse alone sizes it), and the asks for 0 bytes as rows of their own (ZERO): bp_gv_mix
    on ev_syn, ev_ola and lps, the net-scored calls on ev_gain.  A kind that asks for 0 bytes does not size the buffer and leaves its
    block as it was: what the next call finds there is the call's before it.
ev_tab, ev_work and ev_pin stay in UNMODELLED: tab_layout / work_layout of csrc/bp_eval.hip lay out some thirty tables per plan
(resampled lengths, STOI frames and segments, the LPC frame blocks of width 7), which is not short.  The claim made in their place
needs no byte count (width_pairs): in every configuration a scoring call of each width 3 / 5 / 7 at Z or ONE runs directly behind a
dyed L or FULL scoring call of each other width.

Dye.  The new query kinds at L and FULL carry NaN PCM like the old ones.  Read for that, in csrc/: bp_eval_lpc (bp_eval.hip) loops
over a.win, EV_FB and the template order P alone, and a frame of NaN is INVALID by `pos = R[0] > 0.0` / `valid = pos && Rr[0] > 0.0`
(NaN > 0 is false), so it is written as 0.0 with lv = 0; bp_eval_lpcrank reads an invalid frame as +inf, its loop bounds come from
the host's SJ table, every thread counts in ascending order into its own integers, and no NaN is ever compared; bp_eval_lpcsum is
a fixed tree; bp_wave_gv_parts (wave_gv_launch, bp_wave.hip) is one thread per bin, serial over its part's frames in ascending
order; lm_track (bp_classic.h) has "no decision in here: min, max and the clamp only", lm_e1's two loops end at 64 and 200 whatever
the comparison inside says, bp_wave_dnat loops over T from the host's F table.  No data-dependent bound, no result that depends on
the order of arrival: the output under NaN is a function of the input, FINITE_DYE stays empty."""
import collections
import re

import numpy as np

import mix_np as MX
import sequence_model as SM
import size_model as ZM

CAP, D, HOP, CTX = ZM.CAP, ZM.D, ZM.HOP, ZM.CTX
GOOD, DYED, FINITE_DYE = ZM.GOOD, ZM.DYED, ZM.FINITE_DYE
NEW_SIZED = ("gv_mix", "eval_mix_logmmse")
SIZED = ZM.SIZED + list(NEW_SIZED)
UNSIZED = [k for k in SM.XKINDS if k not in SIZED]
EVAL = ("eval_mix",) + NEW_SIZED                               # eval_mix_run
MIXED = ZM.MIXED + NEW_SIZED                                   # generate()
SCORED = ("eval_mix", "eval_mix_logmmse")                      # the kinds with a score width
KEEPS_Y = EVAL                                                 # generate() with a spectrum of the caller's (ev_Y)
NO_Y = ("train_mix", "cv_mix", "mix_features")                 # generate() without: in dynamic mode Y lies behind the nat rows
STATIC, DYNAMIC = 0, 1
NAT_SIZES = ("Z", "M", "L")                                    # the closed nat walk (ONE and FULL: full_walk, the random walks)
# the kinds whose nat_b follows the mode: sequence_model.READS_NAT, and bp_eval_mix_logmmse, which goes through generate() too
# (its scores do not read the rows; the tracker still writes them, one per frame)
ASKS_NAT = SM.READS_NAT + ("eval_mix_logmmse",)


def sizes_of(kind):
    if kind in NEW_SIZED:
        return list(ZM.SIZES)
    return ZM.sizes_of(kind)


def shape(cfg, kind, size, nb=None):
    if kind in NEW_SIZED:
        return ZM.shape(cfg, "eval_mix", size, nb)._replace(kind=kind)
    if kind in SIZED:
        return ZM.shape(cfg, kind, size, nb)
    return ZM.Shape(kind, None, True, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None)


# ------------------------------------------------------------------ the buffers
al256, grown, POLICY = ZM.al256, ZM.grown, ZM.POLICY


def ZERO(s):
    """An ask for 0 bytes that the call site spells out (wave_grow leaves the block as it is)."""
    return 0


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
    [(k, ("bp_step.hip", lambda s: s.n_nat * D * 4, lambda s: s.n_nat * D * 4)) for k in ZM.WINDOWS] +     # the caller's rows, either mode
    [(k, ("bp_mix.hip", _per_sentence, lambda s: y_tail(s) + s.n * D * 8)) for k in NO_Y] +
    [(k, ("bp_mix.hip", _per_sentence, _per_frame)) for k in KEEPS_Y] +
    [("enhance", ("bp_wave.hip", _per_sentence, _per_frame)), ("stream", ("bp_stream.hip", _per_sentence, _per_frame))])


def _nat_ask(s):
    return NAT_ASK[s.kind][2 if s.dyn else 1](s)


def _static_nat_ask(s):
    """size_model's row: the static ask whatever the mode (the mutant of the coverage test)."""
    return s.n_nat * D * 4


Buffer, _ask, _merge = ZM.Buffer, ZM._ask, ZM._merge


def _extend(row, kinds, fn):
    return row._replace(ask=_merge(row.ask, _ask(kinds, fn)))


def _buffers():
    B = collections.OrderedDict(ZM.BUFFERS)
    like = lambda name, kind: B[name].ask[kind]
    B["wset.r[0]"] = _extend(B["wset.r[0]"], NEW_SIZED, like("wset.r[0]", "eval_mix"))
    B["wset.r[2]"] = B["wset.r[2]"]._replace(ask=_ask(list(NAT_ASK), _nat_ask))
    B["wset.r[3]"] = _extend(B["wset.r[3]"], NEW_SIZED, like("wset.r[3]", "eval_mix"))
    for name in ("out_chunk", "host_out"):                     # (`if (!lm ...) out_chunk_reserve`: the log-MMSE call runs no net)
        B[name] = _extend(B[name], ("gv_mix",), like(name, "eval_mix"))
    for name in ("in_d", "x", "s", "v", "gain", "in_pin"):
        B[name] = _extend(B[name], NEW_SIZED, like(name, "eval_mix"))
    B["lps"] = _extend(_extend(B["lps"], ("eval_mix_logmmse",), like("lps", "eval_mix")), ("gv_mix",), ZERO)
    B["ev_Y"] = _extend(B["ev_Y"], NEW_SIZED, like("ev_Y", "eval_mix"))
    for name in ("ev_syn", "ev_ola"):
        B[name] = _extend(_extend(B[name], ("eval_mix_logmmse",), like(name, "eval_mix")), ("gv_mix",), ZERO)
    B["ev_lps"] = _extend(_extend(B["ev_lps"], ("eval_mix_logmmse",), like("ev_lps", "eval_mix")), ("gv_mix",), lambda s: al256(s.n * D * 4))
    B["ev_gain"] = Buffer("ev_gain", "grow", 1, "wave_grow:eval", _merge(_ask(("eval_mix_logmmse",), lambda s: s.n * (D + 1) * 4),
                                                                         _ask(("eval_mix", "gv_mix"), ZERO)))
    return B


BUFFERS = _buffers()
UNMODELLED = collections.OrderedDict((k, v) for k, v in ZM.UNMODELLED.items() if k != "ev_gain")
NEVER = ZM.NEVER
# the buffers whose ask depends on the mode or on WHICH kind of a site makes the call (the coverage test makes its claims for these)
BY_MODE = ("wset.r[2]",)
BY_KIND = ("lps", "ev_syn", "ev_ola", "ev_lps", "ev_gain")
# (kind, buffer, mode) cells among the NEW ones -- the new sized kinds, and every kind's dynamic ask -- that L does NOT regrow behind M
# although the buffer can regrow, and why: none.  (size_model.L_EXEMPT's one cell, a stream's static nat rows, stays there; in
# dynamic mode a stream asks for a row per frame due, 520 at L.)
L_EXEMPT = {}


class _View(object):
    def __init__(self, s, sL, dyn):
        self.__dict__.update(s._asdict(), sL=sL, dyn=dyn)


def asks(cfg, name, s, nat=STATIC, buffers=None):
    """What call s asks buffer `name` for in noise-aware mode `nat` (0: it does not size it)."""
    b = (buffers or BUFFERS)[name]
    fn = b.ask.get(s.kind)
    if fn is None or (not s.ok and not (s.open_frames and b.policy == "frames")):
        return 0
    return int(fn(_View(s, ZM.sl_of(cfg), bool(nat))))


def sizing_kinds(name, buffers=None):
    return [k for k, fn in (buffers or BUFFERS)[name].ask.items() if fn is not ZERO]


def zero_kinds(name, buffers=None):
    return [k for k, fn in (buffers or BUFFERS)[name].ask.items() if fn is ZERO]


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
    known = set(b.member for b in buffers.values()) | set(unmodelled) | set(ZM.OTHER_BUFS)
    out = ["a Buf without a row: %s" % m for m in sorted(found["members"] - known)]
    out += ["a row for a Buf the sources no longer hold: %s" % m for m in sorted(known - found["members"])]
    table = set(b.member for b in buffers.values() if b.site.startswith("wave_grow")) | set(unmodelled)
    out += ["wave_grow sizes %s, which no row names" % m for m in sorted(found["grown_args"] - table)]
    out += ["a wave_grow row for %s, which no wave_grow call lists" % m for m in sorted(table - found["grown_args"])]
    if found["sites"] != ZM.SITES:
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


# ------------------------------------------------------------------ the model
Step = ZM.Step
_PROBE = {}


def _leaves(kind):
    if kind not in _PROBE:
        st = SM.fresh_state()
        SM.XKINDS[kind].apply(SM.XCONFIGS[0], st, 0)
        _PROBE[kind] = (st["windows"], st["has_targ"])
    return _PROBE[kind]


def run_model(cfg, calls, st=None):
    """The model over calls = [(pos, kind, size), ...] from a fresh handle: sequence_model.x_run_model with sizes.  A sized call is
    refused for its size first (the capacity is checked with the plan, before the switches are read)."""
    st = SM.fresh_state() if st is None else dict(st)
    out = []
    for pos, kind, size in calls:
        k = SM.XKINDS[kind]
        before = dict(st)
        if kind in SIZED:
            s = shape(cfg, kind, size)
            why = k.pre(cfg, st, pos) if s.ok else "over"
            status = SM.BP_ERR_ARG if not s.ok else SM.BP_OK if why is None else k.fail[why]
            if status == SM.BP_OK:
                w, t = _leaves(kind)
                SM._resident(st, pos, kind, s.resident, w, t)
                st["bunches"] += s.bunches
        else:
            why = k.pre(cfg, st, pos)
            status = SM.BP_OK if why is None else k.fail[why]
            if why is None:
                k.apply(cfg, st, pos)
        out.append(Step(pos, kind, size, status, before, dict(st)))
    return out


def idle(cfg, step):
    """A successful training call that trains nothing (size Z)."""
    return step.kind in SIZED and SM.XKINDS[step.kind].training and step.status == SM.BP_OK and shape(cfg, step.kind, step.size).bunches == 0


def dyed(kind, size):
    return size in DYED and kind in SIZED and not SM.XKINDS[kind].training


def width_of(cfg, step):
    return SM.choice(cfg, step.pos, step.kind)["width"] if step.kind in SCORED else None


# ------------------------------------------------------------------ the walks
EV_KINDS = ("eval_mix", "gv_mix", "eval_mix_logmmse", "mix_features")    # the kinds of the ev_* buffers and the fourth that sizes lps
NAT_KINDS = SM.READS_NAT
# Pieces per closed walk, each a GPU test of its own from fresh handles (the rule of sequence_model.pieces).  Chosen from the
# measured seconds of one run with 4 and 12 pieces (up to 17.2 s per whole ev walk and 62.8 s per whole nat walk,
# slowest piece 6.95 s), so that the slowest piece of that day stays a factor of two under ten seconds.
N_PIECES = collections.OrderedDict([("ev", 6), ("nat", 20)])
N_RANDOM, RANDOM_LEN = 4, 60
# the first seed at which width_pairs holds in all four configurations
EV_SEED = 40
WALK_NO = {"ev": 20, "nat": 21, "xover": 22, "xfull": 23, "xmeasure": 24, "xrandom": 29, "xregrow": 33}     # behind both models' numbers
MEASURE_SIZES = GOOD


def ev_nodes(cfg):
    return [(k, z) for k in EV_KINDS for z in GOOD]


def nat_nodes(cfg):
    return [(k, z, m) for k in NAT_KINDS for z in NAT_SIZES for m in (STATIC, DYNAMIC)]


def nodes(cfg, fid):
    return ev_nodes(cfg) if fid == "ev" else nat_nodes(cfg)


def closed_walk(cfg, fid, seed=None):
    """One closed walk that takes every ordered pair of the family's nodes once (sequence_model._circuit on the nodes)."""
    ns = nodes(cfg, fid)
    salt = (EV_SEED if seed is None else seed) if fid == "ev" else 0
    return [ns[i] for i in SM._circuit(len(ns), [cfg.index, 31, list(N_PIECES).index(fid), salt])]


def _with_modes(seq, nat=STATIC):
    """[(node index, kind, size, mode)] -> calls: pos = 2 * index for the node, 2 * index - 1 for the set_nat in front of it where the
    node's mode is not the handle's (a stream opens inside its call, so behind the set_nat)."""
    out = []
    for i, k, z, m in seq:
        if m != nat:
            out.append((2 * i - 1, "set_nat", None))
            nat = m
        out.append((2 * i, k, z))
    return out


def pieces(cfg, fid, n_pieces=None, seed=None):
    """The calls per piece; a piece starts with the call that the one before it ended with, from a fresh handle (static mode)."""
    P = N_PIECES[fid] if n_pieces is None else n_pieces
    w = closed_walk(cfg, fid, seed)
    n = len(w) - 1
    cuts = [round(i * n / P) for i in range(P + 1)]
    out = []
    for i in range(P):
        idx = range(cuts[i], cuts[i + 1] + 1)
        if fid == "ev":
            out.append([(p,) + w[p] for p in idx])
        else:
            out.append(_with_modes([(p,) + w[p] for p in idx]))
    return out


def piece_nodes(cfg, fid, n_pieces=None):
    """The nodes per piece (for the nat family with their modes), as the model runs them."""
    out = []
    for p in pieces(cfg, fid, n_pieces):
        steps = run_model(cfg, p)
        out.append([(s.kind, s.size) if fid == "ev" else (s.kind, s.size, s.before["nat"]) for s in steps if s.kind != "set_nat"])
    return out


def over_walk(cfg):
    """OVER once behind every other size of its kind: the two new sized kinds in static mode, then every kind whose noise-aware rows
    follow the mode in DYNAMIC mode."""
    seq = []
    for m, kinds in ((STATIC, NEW_SIZED), (DYNAMIC, ASKS_NAT)):
        for k in kinds:
            for z in sizes_of(k):
                if z != "OVER":
                    seq += [(k, z, m), (k, "OVER", m)]
    return _with_modes([(i + 1,) + n for i, n in enumerate(seq)]) + [(2 * len(seq) + 2, "checkpoint", None)]


def full_walk(cfg):
    """ONE and FULL in dynamic mode, which the closed nat walk leaves out, by construction: per kind ONE and FULL in dynamic mode, Z
    in static mode behind it, FULL in static mode, Z in dynamic mode behind it."""
    seq = []
    for k in ASKS_NAT:
        seq += [(k, "ONE", DYNAMIC), (k, "FULL", DYNAMIC), (k, "Z", STATIC), (k, "FULL", STATIC), (k, "Z", DYNAMIC)]
    return _with_modes([(i + 1,) + n for i, n in enumerate(seq)]) + [(2 * len(seq) + 2, "checkpoint", None)]


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


def measure_walk(cfg, size):
    """A stacked chunk of `size` in front of time_kernel, then every training kind, then a checkpoint; the same with profile_step
    behind a chunk with targets (a window chunk); and behind a time_kernel one query of the out_chunk family at L, so that the
    call after a timing run regrows what it may overwrite.  Kernel ids by position (sequence_model.choice)."""
    out = []
    for i, t in enumerate(SM.TRAINING_KINDS):
        tz = (t, "M" if t in SIZED else None)
        out += [("train" if i % 2 == 0 else "upload_train", size), ("time_kernel", None), tz, ("checkpoint", None),
                ("train", size), ("time_kernel", None), (_OUT_QUERIES[i], "L"),
                ("train_windows", size), ("profile_step", None), tz, ("checkpoint", None)]
    return [(p,) + n for p, n in enumerate(out)]


def x_kinds_of(cfg):
    return SM.x_kinds_of(cfg)


def random_walk(cfg, seed):
    """A kind of the extended table at random, then one of its sizes (OVER among them)."""
    ks = x_kinds_of(cfg)
    rng = np.random.default_rng([cfg.index, 4000 + seed])
    out = []
    for p in range(RANDOM_LEN):
        k = ks[int(rng.integers(len(ks)))]
        zs = sizes_of(k) if k in SIZED else [None]
        out.append((p, k, zs[int(rng.integers(len(zs)))]))
    return out


def walk_ids(cfg):
    return (["%s%d" % (f, i) for f, P in N_PIECES.items() for i in range(P)] + ["xover", "xfull", "xregrow"] +
            ["xmeasure%s" % z for z in MEASURE_SIZES] + ["xrandom%d" % s for s in range(N_RANDOM)])


def walk_calls(cfg, wid):
    """(walk number for the data, calls) of one walk id."""
    for f in N_PIECES:
        if wid.startswith(f) and wid[len(f):].isdigit():
            return WALK_NO[f], pieces(cfg, f)[int(wid[len(f):])]
    if wid == "xover":
        return WALK_NO["xover"], over_walk(cfg)
    if wid == "xfull":
        return WALK_NO["xfull"], full_walk(cfg)
    if wid == "xregrow":
        return WALK_NO["xregrow"], regrow_walk(cfg)
    if wid.startswith("xmeasure"):
        z = wid[len("xmeasure"):]
        return WALK_NO["xmeasure"] + MEASURE_SIZES.index(z), measure_walk(cfg, z)
    s = int(wid[len("xrandom"):])
    return WALK_NO["xrandom"] + s, random_walk(cfg, s)


def test_id(cfg, wid):
    return "tests/test_xsize_gpu.py::test_xsize_walk[%s-%s]" % (cfg.id, wid)


GPU_TESTS = [test_id(c, w) for c in SM.XCONFIGS for w in walk_ids(c)]


def pair_table(cfg, fid, n_pieces=None):
    """(node, next node) -> the GPU tests that run it."""
    out = {}
    for i, p in enumerate(piece_nodes(cfg, fid, n_pieces)):
        for a, b in zip(p, p[1:]):
            out.setdefault((a, b), []).append(test_id(cfg, "%s%d" % (fid, i)))
    return out


def all_walks(cfg):
    return [(wid,) + walk_calls(cfg, wid) for wid in walk_ids(cfg)]


def width_pairs(cfg, calls):
    """(width of a dyed L or FULL scoring call, width of the scoring call at Z or ONE directly behind it), both successful."""
    steps = run_model(cfg, calls)
    return set((width_of(cfg, a), width_of(cfg, b)) for a, b in zip(steps, steps[1:])
               if a.kind in SCORED and b.kind in SCORED and a.size in DYED and b.size in ("Z", "ONE") and a.status == b.status == SM.BP_OK)


WIDTH_PAIRS = set((a, b) for a in SM.WIDTHS for b in SM.WIDTHS if a != b)


def ev_seed_holds(seed):
    return all(set().union(*[width_pairs(c, p) for p in pieces(c, "ev", seed=seed)]) >= WIDTH_PAIRS for c in SM.XCONFIGS)


# ------------------------------------------------------------------ what the policy does along a walk
Sim = collections.namedtuple("Sim", "regrows by_mode smaller by_prev zero_behind tail_moves behind_time")


def simulate(cfg, calls, buffers=None):
    """Along one walk from a fresh handle, per buffer:
    regrows      growths of a block that exists (synchronise, free, unzeroed memory)
    by_mode      ... of those that are owed to the mode -- the block was last sized in the OTHER mode, and in that mode this call
                 would have asked for another count of bytes: (mode of the block, mode of the call) -> count
    smaller      (kind, mode) that ran a SMALLER request behind a regrow in the block it left
    by_prev      (kind of the call directly before, kind that regrows the block) -> count
    zero_behind  (kind that asks for 0 bytes and leaves a REGROWN block alone, kind of the call directly before it)
    and over the walk: tail_moves, the NO_Y kinds whose Y tail starts at another byte offset than the dynamic NO_Y call directly
    before them; behind_time, the regrows of out_chunk by the call directly behind a successful time_kernel."""
    B = BUFFERS if buffers is None else buffers
    cap = {n: [0] * b.slots for n, b in B.items()}
    cur = {n: 0 for n in B}
    last = {n: [None] * b.slots for n, b in B.items()}
    regrown = {n: [False] * b.slots for n, b in B.items()}
    regrows, by_mode, by_prev = collections.Counter(), collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    smaller, zero_behind = collections.defaultdict(set), collections.defaultdict(set)
    tail_moves, behind_time = set(), 0
    prev = None
    for step in run_model(cfg, calls):
        if step.kind not in SIZED:
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


def corpus(cfg):
    """sequence_model.x_corpus, extended as size_model.corpus extends sequence_model.corpus: one entry per (frames, dyed) that a size
    needs, in size_model's order (the new sized kinds have eval_mix's sentences and need none of their own).  On D every entry
    behind the first four also gets a reverberated twin, so that the derived entries appear in plans at every size:
    twin[i] is the corpus index of entry i's."""
    if cfg.id not in _CORPUS:
        cor = SM.x_corpus(cfg)
        rng = np.random.default_rng([cfg.index, 97])
        clean, index = list(cor["clean"]), {}
        for T, dy in ZM.corpus_T(cfg):
            index[(T, dy)] = len(clean)
            x = (rng.normal(size=ZM.len_of(T)) * 3000.0).astype(np.float32)
            clean.append(np.full_like(x, np.nan) if dy else x)
        cor.update(clean=clean, index=index, twin={})
        if SM.has_reverb(cfg):
            n0, n = len(SM.CLEAN_LEN), len(clean)
            extra = list(range(n0, n))
            cor["pair_clean"] = list(cor["pair_clean"]) + extra
            cor["pair_rir"] = list(cor["pair_rir"]) + [i % len(cor["rirs"]) for i in range(len(extra))]
            cor["twin"] = dict([(c, n + j) for j, c in enumerate(SM.x_corpus(cfg)["pair_clean"])] +
                               [(c, n + len(SM.REVERB_PAIRS) + j) for j, c in enumerate(extra)])
        _CORPUS[cfg.id] = cor
    return _CORPUS[cfg.id]


def source_of(cfg, entry):
    """The clean entry a plan's index stands for (a derived entry: the sentence it was made from)."""
    cor = corpus(cfg)
    return entry if entry < len(cor["clean"]) else cor["pair_clean"][entry - len(cor["clean"])]


def frames_of_entry(cfg, entry):
    return SM.frames_of(len(corpus(cfg)["clean"][source_of(cfg, entry)]))


def _plan(cfg, rng, kind, size, s):
    cor = corpus(cfg)
    if size == "M":                                            # sequence_model's plans: on D entries 4 and 5 are the derived ones
        clean = SM.x_train_clean(cfg) if kind == "train_mix" else SM.x_query_clean(cfg)
        n0 = len(SM.CLEAN_LEN)
        return SM._plan(rng, [c if c < n0 else len(cor["clean"]) + c - n0 for c in clean])
    dy = dyed(kind, size)
    clean = [cor["index"][(T, dy and not (kind == "mix_features" and i == 0))] for i, T in enumerate(s.T)]
    return SM._plan(rng, [cor["twin"].get(c, c) if i % 2 == 0 else c for i, c in enumerate(clean)])


def call_data(cfg, walk, pos, kind, size):
    """What the call at position pos of walk number `walk` is made with: size_model.call_data for the stacked, window, enhance and
    stream kinds; the mixing kinds from this module's corpus, with what the call asks for beyond its data (sequence_model.choice)."""
    if kind not in SIZED:
        return SM.choice(cfg, pos, kind)
    if kind not in MIXED:
        return ZM.call_data(cfg, walk, pos, kind, size)
    rng = np.random.default_rng([cfg.index, 100 + walk, pos])
    s = shape(cfg, kind, size)
    d = dict(SM.choice(cfg, pos, kind), plan=_plan(cfg, rng, kind, size, s))
    if kind == "train_mix":
        d["order"] = MX.shuffle(1 + pos, 10 * walk + cfg.index, s.n) if s.ok else np.arange(s.n)
    return d


# ------------------------------------------------------------------ the figures of a GPU run
def numbers(parity):
    keep = {k: v for k, v in sorted(parity["tests"].items()) if "test_xsize_gpu.py" in k}
    return {"source": "a -m gpu run of tests/test_xsize_gpu.py on an MI355X; `python tests/xsize_model.py numbers <parity JSON> <out>` behind it",
            "bar": "bit for bit: words_differing == 0 in every entry", "tests": keep}


if __name__ == "__main__":
    import json
    import sys
    if len(sys.argv) == 4 and sys.argv[1] == "numbers":
        json.dump(numbers(json.load(open(sys.argv[2]))), open(sys.argv[3], "w"), indent=1, sort_keys=True)
    elif len(sys.argv) == 2 and sys.argv[1] == "seed":
        print(next(s for s in range(1000) if ev_seed_holds(s)))
    else:
        for cfg in SM.XCONFIGS:
            print(cfg.id, {w: len(c) for w, _, c in all_walks(cfg)})
