"""Host-side mirror of the reference's `BP_GPU` class (BP_GPU.h:40-88) over the C ABI in
include/bp_c_api.h (ctypes binding of libbp_hip.so, the gfx950 HIP library).

Same constructor argument order, method names, argument meaning and error behaviour as the
reference object so callers/tests read like `BPtrain.cc`:

    obj = BP_GPU(gpu_used, numlayers, layersizes, bunchsize, lrate, momentum, weightcost,
                 weights, bias, dropoutflag, visible_omit, hid_omit)
    obj.train(n_frames, indata, targ)             # BP_GPU.cu:241-331
    err = obj.CrossValid(n_frames, indata, targ)  # BP_GPU.cu:408-479 (SUM of squared errors)
    obj.returnWeights(weights, bias)              # BP_GPU.cu:910-923

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible the
constructor raises.  (The reference prints and calls exit(0) on errors, BP_GPU.cu:20-24;
`strict_exit=True` reproduces that, the default raises BPError so Python callers can react.)

The ABI itself (signatures, struct mirrors, constants) is _abi.py; the calls that need no handle are signal.py and rbm.py.
"""
import ctypes as C
import sys

import numpy as np

from ._abi import (BPConfig, BPError, BPMelParams, BPMixCorpus, BPMixReverb, BPStreamConfig, BPWaveChunk, BPWindowChunk, Closing,
                   FORWARD_DEFAULT, GV_STAGES, MAXLAYER, MIX_LPS, MIX_TARGETS, MIXTURE_DTYPE, NAT_MODES, PROF_KINDS, REVERB_TARGETS,
                   WAVE_LPS, check, flat32, load_library, pack, ptr, ptrs, score_columns, split)
from .signal import logmmse_params, noise_params, post_params, stream_push

__all__ = ["BP_GPU", "Stream", "Rendezvous", "device_count", "device_pci_bus_id"]


class BP_GPU(Closing):
    """Drop-in for the reference trainer object; see module docstring."""

    def __init__(self, gpu_used, numlayers, layersizes, bunchsize, lrate, momentum, weightcost, weights, bias,
                 dropoutflag=0, visible_omit=0.0, hid_omit=0.0, activation=0, momentum_rule=0, seed=0, device=0,
                 global_bunchsize=0, rank_frame_offset=0, max_chunk_frames=0, strict_exit=False, compute_dtype=0,
                 output_activation=0, output_linear_cols=0, output_loss=0, forward_mode=FORWARD_DEFAULT, nat_mode="static",
                 nat_noise=None):
        self._h = None
        self._strict = strict_exit
        self._lib = load_library()
        self.numlayers = int(numlayers)
        self.layersizes = [int(x) for x in list(layersizes)[:numlayers]]
        self.bunchsize = int(bunchsize)
        self.lrate, self.momentum, self.weightcost = float(lrate), float(momentum), float(weightcost)
        self.dropoutflag, self.visible_omit, self.hid_omit = int(dropoutflag), float(visible_omit), float(hid_omit)
        cfg = BPConfig()
        cfg.gpu_used, cfg.numlayers, cfg.bunchsize = int(gpu_used), self.numlayers, self.bunchsize
        for i, s in enumerate(self.layersizes[:MAXLAYER]):
            cfg.layersizes[i] = s
        cfg.lrate, cfg.momentum, cfg.weightcost = self.lrate, self.momentum, self.weightcost
        cfg.dropoutflag, cfg.visible_omit, cfg.hid_omit = self.dropoutflag, self.visible_omit, self.hid_omit
        cfg.activation, cfg.momentum_rule, cfg.seed, cfg.device = int(activation), int(momentum_rule), int(seed), int(device)
        cfg.global_bunchsize, cfg.rank_frame_offset = int(global_bunchsize), int(rank_frame_offset)
        cfg.max_chunk_frames = int(max_chunk_frames)
        cfg.compute_dtype = int(compute_dtype)          # 0 fp32 (reference) | 1 bf16 operands, fp32 accumulate / master weights
        self._cfg = cfg
        if len(self.layersizes) != self.numlayers or self.numlayers < 2 or self.numlayers > MAXLAYER - 1:
            self._fail("numlayers must be in 2..%d and match layersizes" % (MAXLAYER - 1))
        w = [None] * MAXLAYER
        b = [None] * MAXLAYER
        for l in range(1, self.numlayers):
            w[l] = np.ascontiguousarray(weights[l], dtype=np.float32).reshape(-1)
            b[l] = np.ascontiguousarray(bias[l], dtype=np.float32).reshape(-1)
            if w[l].size != self.layersizes[l - 1] * self.layersizes[l] or b[l].size != self.layersizes[l]:
                self._fail("weights[%d]/bias[%d] have the wrong size" % (l, l))
        out_mode = self._output_args(output_activation, output_linear_cols, output_loss)
        self.output_activation = self.output_linear_cols = self.output_loss = 0
        h = C.c_void_p()
        self._check(self._lib.bp_create(C.byref(cfg), ptrs(w), ptrs(b), C.byref(h)))
        self._h = h
        self.forward_mode = FORWARD_DEFAULT
        if out_mode != (0, 0, 0):
            self.set_output(*out_mode)
        if int(forward_mode) != FORWARD_DEFAULT:
            self.set_forward(forward_mode)
        self._nat_mode = "static"
        self._mix_aux = self._mix_aux_set = None
        if nat_mode != "static" or nat_noise is not None:
            self.set_nat(nat_mode, nat_noise)

    # ------------------------------------------------------------------ errors
    def _fail(self, msg):
        if self._strict:                      # reference convention: printf + exit(0)
            print(msg)
            sys.exit(0)
        raise BPError(msg)

    def _check(self, rc):
        if rc != 0:
            try:
                check(self._lib, rc)
            except BPError as e:
                self._fail(str(e))

    def _in(self, a, n_frames, width, name):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size < n_frames * width:
            self._fail("%s holds %d floats, need %d" % (name, a.size, n_frames * width))
        return a

    # ------------------------------------------------------------------ reference API
    def _push_hyper(self):
        """The reference reads its public members afresh on every bunch (BP_GPU.cu:488-500): a caller may
        assign obj.lrate / momentum / weightcost / dropoutflag / visible_omit / hid_omit between chunks.  Every method that runs
        the net pushes them first -- training, CV and gradients, and also the forwards (forward, enhance_waves, eval_mix, a
        stream's push: the keep-scale follows dropoutflag and the omit rates) -- so that what a call computes does not depend
        on which method was called before it."""
        self._check(self._lib.bp_set_hyper(self._h, float(self.lrate), float(self.momentum), float(self.weightcost),
                                           int(self.dropoutflag), float(self.visible_omit), float(self.hid_omit)))

    def _output_args(self, activation, linear_cols, loss):
        """Checks of bp_set_output, made here so that a bad value never reaches the library."""
        a, c, s = int(activation), int(linear_cols), int(loss)
        if a not in (0, 1):
            self._fail("output activation must be 0 (linear) or 1 (logistic)")
        if s not in (0, 1):
            self._fail("output loss must be 0 (cross-entropy) or 1 (squared error)")
        if a == 0 and (c != 0 or s != 0):
            self._fail("output linear_cols and loss must be 0 with the linear output")
        if a == 1 and not 0 <= c < self.layersizes[-1]:
            self._fail("output linear_cols must be in [0, %d) with the logistic output" % self.layersizes[-1])
        return a, c, s

    def set_output(self, activation, linear_cols=0, loss=0):
        """Output-layer nonlinearity (bp_set_output): 0 linear; 1 logistic on the output columns [linear_cols, sL), trained
        with loss 0 (cross-entropy: dEdz = 2/Bg (y - t)) or 1 (squared error through the logistic).  From the next call on."""
        a, c, s = self._output_args(activation, linear_cols, loss)
        self._check(self._lib.bp_set_output(self._h, a, c, s))
        self.output_activation, self.output_linear_cols, self.output_loss = a, c, s

    def set_forward(self, mode):
        """The kernels of the inference forward (bp_set_forward): FORWARD_DEFAULT, or FORWARD_ROWINV -- a frame's output bits then
        depend on its input row and the net alone, and streams opened from now on pack their channels.  fp32 handles."""
        self._check(self._lib.bp_set_forward(self._h, int(mode)))
        self.forward_mode = int(mode)

    def set_nat(self, mode, noise=None):
        """The noise-aware block of the calls that stage it (bp_set_nat): "static", one row per sentence (the default), or
        "dynamic", one row per frame from the MMSE-SPP noise tracker -- enhance_waves, train_mix, CrossValid_mix, mix_features
        and eval_mix from the next call on, and the streams opened from now on (an open stream keeps its mode).  noise: what noise_params takes (None: the tracker's defaults)."""
        if mode not in NAT_MODES:
            self._fail("set_nat: mode must be \"static\" or \"dynamic\", not %r" % (mode,))
        try:
            nz = noise_params(noise)
        except BPError as e:
            self._fail(str(e))
        self._check(self._lib.bp_set_nat(self._h, NAT_MODES[mode], C.byref(nz)))
        self._nat_mode = mode

    @property
    def nat_mode(self):
        """"static" or "dynamic": what set_nat (or nat_mode= at construction) set last."""
        return self._nat_mode

    def set_post(self, gv_center=None, gv_scale=None, mask_col=-1, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0, fea_dim=None):
        """Post-processing of the LPS estimate before resynthesis (bp_set_post): GV equalisation x = c + s (x - c) with gv_center and
        gv_scale (what gv_factors returns), then the mask gate -- the noisy LPS blended in where the mask columns from mask_col on say
        that speech dominates.  enhance_waves and eval_mix from the next call on, and the streams opened from now on.  set_post(None),
        or no argument at all, switches it off.  fea_dim: needed only for gating without GV (default: the corpus's)."""
        if gv_center is None and gv_scale is None and int(mask_col) < 0:
            self._check(self._lib.bp_set_post(self._h, 0, None))
            self._post = False
            return
        try:
            p = post_params(gv_center, gv_scale, mask_col, mask_lo, mask_hi, mask_weight)
        except BPError as e:
            self._fail(str(e))
        D = p._center.size if p.gv else fea_dim if fea_dim is not None else getattr(self, "mix_fea_dim", None)
        if D is None:
            self._fail("set_post: fea_dim is needed for gating without GV on a handle without a corpus")
        self._check(self._lib.bp_set_post(self._h, int(D), C.byref(p)))
        self._post = True

    @property
    def post(self):
        """True while post-processing is on (set_post)."""
        return getattr(self, "_post", False)

    def gv_mix(self, plan, out_col=0, stage="raw"):
        """bp_gv_mix: the second moments the GV factors are made from, over the plan's mixtures: dict of est_sum, est_sq, ref_sum,
        ref_sq (float64 [fea_dim]) and frames.  stage "raw": the net's columns from out_col on; "post": the rows that are
        resynthesised (set_post).  Across plans the caller adds the sums; gv_factors takes the dict."""
        if stage not in GV_STAGES:
            self._fail("gv_mix: stage must be \"raw\" or \"post\", not %r" % (stage,))
        p, pp = self._plan(plan)
        self._push_hyper()
        D = getattr(self, "mix_fea_dim", None) or 1
        out = {k: np.zeros(D, np.float64) for k in ("est_sum", "est_sq", "ref_sum", "ref_sq")}
        n = C.c_int64(0)
        self._check(self._lib.bp_gv_mix(self._h, p.size, pp, int(out_col), GV_STAGES[stage], ptr(out["est_sum"]), ptr(out["est_sq"]),
                                        ptr(out["ref_sum"]), ptr(out["ref_sq"]), C.byref(n)))
        out["frames"] = int(n.value)
        return out

    def set_mix_aux(self, mel):
        """The MFCC auxiliary target of the mixing corpus (bp_set_mix_aux): what mel_params makes, or None for none.  From the next
        set_mix_corpus on -- its target must then begin with LPS and layersizes[-1] be parts * fea_dim + n_ceps; the target row is
        [LPS | MFCC | mask].  A corpus that is already set keeps what it was set with."""
        if mel is not None and not isinstance(mel, BPMelParams):
            self._fail("set_mix_aux: mel must be None or what mel_params returns")
        self._check(self._lib.bp_set_mix_aux(self._h, None if mel is None else C.byref(mel)))
        self._mix_aux = None if mel is None else (int(mel.n_mel), int(mel.n_ceps))

    @property
    def mix_aux_dims(self):
        """(n_mel, n_ceps) of the MFCC columns of the corpus set last, or None when it has none."""
        return self._mix_aux_set

    def train(self, n_frames, indata, targ):
        x = self._in(indata, n_frames, self.layersizes[0], "in")
        t = self._in(targ, n_frames, self.layersizes[-1], "targ")
        self._push_hyper()
        self._check(self._lib.bp_train_chunk(self._h, int(n_frames), ptr(x), ptr(t)))

    def CrossValid(self, n_frames, indata, targ):
        x = self._in(indata, n_frames, self.layersizes[0], "in")
        t = self._in(targ, n_frames, self.layersizes[-1], "targ")
        self._push_hyper()
        e = C.c_float(0.0)
        self._check(self._lib.bp_cv_chunk(self._h, int(n_frames), ptr(x), ptr(t), C.byref(e)))
        return float(e.value)

    def returnWeights(self, weights, bias):
        """Fills caller-owned arrays weights[l]/bias[l], l = 1..numlayers-1 (index 0 unused)."""
        for l in range(1, self.numlayers):
            for a, n in ((weights[l], self.layersizes[l - 1] * self.layersizes[l]), (bias[l], self.layersizes[l])):
                if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.size == n):
                    self._fail("returnWeights: arrays must be contiguous float32 of the layer's size")
        self._check(self._lib.bp_get_weights(self._h, ptrs(weights), ptrs(bias)))

    # ------------------------------------------------------------------ conveniences / extensions
    def _new_params(self):
        w = [None] + [np.empty((self.layersizes[l - 1], self.layersizes[l]), np.float32) for l in range(1, self.numlayers)]
        b = [None] + [np.empty(self.layersizes[l], np.float32) for l in range(1, self.numlayers)]
        return w, b

    def get_weights(self):
        w, b = self._new_params()
        self.returnWeights(w, b)
        return w, b

    def get_deltas(self):
        w, b = self._new_params()
        self._check(self._lib.bp_get_deltas(self._h, ptrs(w), ptrs(b)))
        return w, b

    def forward(self, indata):
        x = np.ascontiguousarray(indata, dtype=np.float32).reshape(-1, self.layersizes[0])
        out = np.empty((x.shape[0], self.layersizes[-1]), np.float32)
        self._push_hyper()
        self._check(self._lib.bp_forward(self._h, x.shape[0], ptr(x), ptr(out)))
        return out

    def upload_chunk(self, indata, targ):
        x = np.ascontiguousarray(indata, dtype=np.float32).reshape(-1, self.layersizes[0])
        t = self._in(targ, x.shape[0], self.layersizes[-1], "targ")
        self._check(self._lib.bp_upload_chunk(self._h, x.shape[0], ptr(x), ptr(t)))

    # ---- on-device frame stacking (bp_window_chunk): sample i = fea[win_start[i] : win_start[i]+context] (+ nat[nat_row[i]])
    def _windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        fea = np.ascontiguousarray(fea, dtype=np.float32)
        if fea.ndim != 2:
            self._fail("windows: fea must be [n_frames][fea_dim]")
        tg = np.ascontiguousarray(targ_frames, dtype=np.float32).reshape(fea.shape[0], self.layersizes[-1])
        ws = np.ascontiguousarray(win_start, dtype=np.int32)
        tf = np.ascontiguousarray(targ_frame, dtype=np.int32)
        c = BPWindowChunk()
        c.n_samples, c.n_frames, c.fea_dim, c.context = int(ws.size), int(fea.shape[0]), int(fea.shape[1]), int(context)
        c.fea, c.targ_frames, c.win_start, c.targ_frame = ptr(fea), ptr(tg), ptr(ws), ptr(tf)
        keep = [fea, tg, ws, tf]
        if nat is not None:
            nat = np.ascontiguousarray(nat, dtype=np.float32).reshape(-1, fea.shape[1])
            nr = np.ascontiguousarray(nat_row, dtype=np.int32)
            c.n_nat, c.nat, c.nat_row = int(nat.shape[0]), ptr(nat), ptr(nr)
            keep += [nat, nr]
        return c, keep

    def upload_chunk_windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        c, keep = self._windows(fea, targ_frames, context, win_start, targ_frame, nat, nat_row)
        self._check(self._lib.bp_upload_chunk_windows(self._h, C.byref(c)))

    def train_windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        c, keep = self._windows(fea, targ_frames, context, win_start, targ_frame, nat, nat_row)
        self._push_hyper()
        self._check(self._lib.bp_train_chunk_windows(self._h, C.byref(c)))

    def CrossValid_windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        c, keep = self._windows(fea, targ_frames, context, win_start, targ_frame, nat, nat_row)
        e = C.c_float(0.0)
        self._push_hyper()
        self._check(self._lib.bp_cv_chunk_windows(self._h, C.byref(c), C.byref(e)))
        return float(e.value)

    # ---- waveform enhancement (bp_enhance_waves; signal definition: include/bp_c_api.h)
    def enhance_waves(self, sentences, mean, inv_std, context, targ_offset, target=WAVE_LPS, out_col=0, return_net=False):
        """Noisy sentences (1-D float32, int16 units) -> enhanced sentences of the same lengths; with return_net also the
        net outputs per frame, one [T_s][layersizes[-1]] array per sentence."""
        mean, inv_std = flat32(mean), flat32(inv_std)
        D = mean.size
        if inv_std.size != D:
            self._fail("enhance_waves: mean and inv_std differ in length")
        pcm, lens, frames = pack(sentences, D)
        c = BPWaveChunk()
        c.n_sent, c.sent_len, c.pcm = len(lens), ptr(lens), ptr(pcm)
        c.context, c.targ_offset, c.mean, c.inv_std = int(context), int(targ_offset), ptr(mean), ptr(inv_std)
        c.target, c.out_col = int(target), int(out_col)
        out = np.empty(max(pcm.size, 1), np.float32)
        net = np.empty((max(int(frames.sum()), 1), self.layersizes[-1]), np.float32) if return_net else None
        self._push_hyper()
        self._check(self._lib.bp_enhance_waves(self._h, D, C.byref(c), ptr(out), ptr(net)))
        waves = split(out, lens)
        return (waves, split(net, frames)) if return_net else waves

    # ---- streaming sessions (bp_stream_open ...; contract: include/bp_c_api.h)
    def stream_open(self, mean, inv_std, context, targ_offset, target=WAVE_LPS, out_col=0, n_chan=1, max_push_samples=16000):
        """A Stream of n_chan channels on this handle: push(blocks, end) returns the samples that became final, the same bits as
        enhance_waves on the finished sentences.  Close it (or the handle) when done."""
        mean, inv_std = flat32(mean), flat32(inv_std)
        if inv_std.size != mean.size:
            self._fail("stream_open: mean and inv_std differ in length")
        c = BPStreamConfig()
        c.fea_dim, c.context, c.targ_offset, c.mean, c.inv_std = mean.size, int(context), int(targ_offset), ptr(mean), ptr(inv_std)
        c.target, c.out_col, c.n_chan, c.max_push_samples = int(target), int(out_col), int(n_chan), int(max_push_samples)
        s = C.c_void_p()
        self._check(self._lib.bp_stream_open(self._h, C.byref(c), C.byref(s)))
        return Stream(self, s, mean.size, int(context), int(targ_offset), int(n_chan), bool(self._lib.bp_stream_packed(s)),
                      self._nat_mode, self.post)

    # ---- training mixtures made on the device (bp_set_mix_corpus ...; definition: include/bp_c_api.h)
    def set_mix_corpus(self, clean, noise, mean, inv_std, context, targ_offset, target=MIX_LPS, lc_db=5.0):
        """clean, noise: lists of 1-D arrays (int16 units), uploaded once; target: MIX_* or a name of MIX_TARGETS."""
        mean, inv_std = flat32(mean), flat32(inv_std)
        if inv_std.size != mean.size:
            self._fail("set_mix_corpus: mean and inv_std differ in length")
        target = MIX_TARGETS[target] if isinstance(target, str) else int(target)
        cpcm, clen, _ = pack(clean, lens=np.int64)
        npcm, nlen, _ = pack(noise, lens=np.int64)
        c = BPMixCorpus()
        c.fea_dim, c.context, c.targ_offset, c.target, c.lc_db = mean.size, int(context), int(targ_offset), target, float(lc_db)
        c.mean, c.inv_std = ptr(mean), ptr(inv_std)
        c.n_clean, c.clean_len, c.clean_pcm = len(clen), ptr(clen), ptr(cpcm)
        c.n_noise, c.noise_len, c.noise_pcm = len(nlen), ptr(nlen), ptr(npcm)
        self._check(self._lib.bp_set_mix_corpus(self._h, C.byref(c)))
        self.mix_fea_dim, self.mix_clean_len = mean.size, clen
        self.mix_nat = self.layersizes[0] == (int(context) + 1) * mean.size
        self.mix_n_clean, self.mix_reverb_entries = len(clen), 0
        self._mix_aux_set = self._mix_aux

    def set_mix_reverb(self, rirs, pair_clean, pair_rir, target="reverberant", early_taps=0):
        """bp_set_mix_reverb: pair k = (clean sentence pair_clean[k], response rirs[pair_rir[k]]) becomes clean entry n_clean + k
        of the corpus; target: "reverberant" | "early" (REVERB_TARGETS) or the number; replaces the entries of an earlier call."""
        target = REVERB_TARGETS[target] if isinstance(target, str) else int(target)
        hpcm, hlen, _ = pack(rirs)
        pc = np.ascontiguousarray(pair_clean, dtype=np.int32).reshape(-1)
        pr = np.ascontiguousarray(pair_rir, dtype=np.int32).reshape(-1)
        if pc.size != pr.size:
            self._fail("set_mix_reverb: pair_clean and pair_rir differ in length")
        r = BPMixReverb()
        r.n_rir, r.rir_len, r.rir_pcm = len(hlen), ptr(hlen), ptr(hpcm)
        r.n_pair, r.pair_clean, r.pair_rir = pc.size, ptr(pc), ptr(pr)
        r.target, r.early_taps = target, int(early_taps)
        self._check(self._lib.bp_set_mix_reverb(self._h, C.byref(r)))
        n = self.mix_n_clean
        self.mix_clean_len = np.concatenate([self.mix_clean_len[:n], self.mix_clean_len[:n][pc]])
        self.mix_reverb_entries = int(pc.size)

    def _plan(self, plan):
        p = np.ascontiguousarray(plan, dtype=MIXTURE_DTYPE).reshape(-1)
        return p, p.ctypes.data_as(C.c_void_p)

    def mix_frames(self, plan):
        """Frames of every mixture of the plan (T = (len_c - 1)/hop + 2), per the corpus set last."""
        p = np.ascontiguousarray(plan, dtype=MIXTURE_DTYPE).reshape(-1)
        if getattr(self, "mix_fea_dim", None) is None:
            self._fail("mix_frames: no corpus (set_mix_corpus)")
        lens = self.mix_clean_len[p["clean"]]
        return (lens - 1) // (self.mix_fea_dim - 1) + 2

    def train_mix(self, plan, order=None):
        p, pp = self._plan(plan)
        self._push_hyper()
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        if o is not None and o.size != int(self.mix_frames(p).sum()):     # (the library reads sum(T) entries)
            self._fail("train_mix: order must have one entry per frame of the plan (%d), not %d" % (int(self.mix_frames(p).sum()), o.size))
        self._check(self._lib.bp_train_mix(self._h, p.size, pp, ptr(o)))

    def CrossValid_mix(self, plan):
        p, pp = self._plan(plan)
        self._push_hyper()
        e = C.c_float(0.0)
        self._check(self._lib.bp_cv_mix(self._h, p.size, pp, C.byref(e)))
        return float(e.value)

    def mix_features(self, plan):
        """dict of fea [sum T][D] (normalised), lps [sum T][D] (noisy), targ [sum T][sL], nat [n_mix][D] (None without the
        noise-aware block; in nat_mode "dynamic" [sum T][D], the row of every frame) and pcm [sum len_c] (the mixed samples),
        unshuffled."""
        p, pp = self._plan(plan)
        D = getattr(self, "mix_fea_dim", None)
        if D is None:                                   # no corpus: the library reports the state error
            self._check(self._lib.bp_mix_features(self._h, p.size, pp, None, None, None, None, None))
        T = int(self.mix_frames(p).sum())
        n_pcm = int(self.mix_clean_len[p["clean"]].sum())
        has_nat = self.mix_nat
        out = {"fea": np.empty((T, D), np.float32), "lps": np.empty((T, D), np.float32),
               "targ": np.empty((T, self.layersizes[-1]), np.float32),
               "nat": np.empty((T if self._nat_mode == "dynamic" else p.size, D), np.float32) if has_nat else None, "pcm": np.empty(max(n_pcm, 1), np.float32)}
        self._check(self._lib.bp_mix_features(self._h, p.size, pp, ptr(out["fea"]), ptr(out["lps"]), ptr(out["targ"]),
                                              ptr(out["nat"]), ptr(out["pcm"])))
        out["pcm"] = out["pcm"][:n_pcm]
        return out

    def _eval(self, p, ns, return_pcm, call, *args):
        """What eval_mix and eval_mix_logmmse share: the score buffers of ns columns and, with return_pcm on a handle that has a
        corpus, the sample buffer -- the last three arguments of every bp_eval_mix* call, behind args -- and the result."""
        noisy = np.empty((max(p.size, 1), ns), np.float32)
        enh = np.empty((max(p.size, 1), ns), np.float32)
        pcm = lens = None
        if return_pcm and getattr(self, "mix_fea_dim", None) is not None:
            lens = self.mix_clean_len[p["clean"]] if p.size else np.zeros(0, np.int64)
            pcm = np.empty(max(int(lens.sum()), 1), np.float32)
        self._check(call(*(args + (ptr(noisy), ptr(enh), ptr(pcm)))))
        return {"noisy": noisy[:p.size], "enhanced": enh[:p.size], "pcm": None if pcm is None else split(pcm, lens)}

    def eval_mix(self, plan, sample_rate, target=WAVE_LPS, out_col=0, return_pcm=False, extended=False):
        """bp_eval_mix: the plan's mixtures made on the device, enhanced with this net and scored against their clean sentences.
        dict of noisy [n_mix][3] and enhanced [n_mix][3] float32 scores (columns SCORE_SSNR, SCORE_LSD, SCORE_STOI; NaN where
        undefined) and pcm: the enhanced sentences (a list) with return_pcm, else None.  extended: bp_eval_mix_ext with five
        columns, SCORE_ESTOI and SCORE_SISDR behind the same three; extended="full": seven, SCORE_LLR and SCORE_CD behind those;
        extended="all": nine, SCORE_FWSSNR and SCORE_WSS behind those (any other value: BPError)."""
        ns = score_columns("eval_mix", extended)
        p, pp = self._plan(plan)
        self._push_hyper()
        args = (self._h, p.size, pp, int(sample_rate), int(target), int(out_col))
        if ns != 3:
            return self._eval(p, ns, return_pcm, self._lib.bp_eval_mix_ext, *(args + (ns,)))
        return self._eval(p, 3, return_pcm, self._lib.bp_eval_mix, *args)

    def eval_mix_logmmse(self, plan, sample_rate, params=None, return_pcm=False, extended=False, noise=None):
        """bp_eval_mix_logmmse: eval_mix with the log-MMSE baseline in place of the net (params: None for the defaults, a dict of
        bp_logmmse_params fields over them, or a BPLogmmseParams).  The same dictionary as eval_mix (extended: five columns, "full":
        seven, "all": nine, bp_eval_mix_logmmse_ext).  noise: as for logmmse_waves (anything but None: bp_eval_mix_logmmse_nt)."""
        ns = score_columns("eval_mix_logmmse", extended)
        p, pp = self._plan(plan)
        lm = logmmse_params(params)
        lmp = None if lm is None else C.byref(lm)
        if noise is not None:
            nz = noise_params(noise)
            return self._eval(p, ns, return_pcm, self._lib.bp_eval_mix_logmmse_nt, self._h, lmp, C.byref(nz), p.size, pp, int(sample_rate), ns)
        if ns != 3:
            return self._eval(p, ns, return_pcm, self._lib.bp_eval_mix_logmmse_ext, self._h, lmp, p.size, pp, int(sample_rate), ns)
        return self._eval(p, ns, return_pcm, self._lib.bp_eval_mix_logmmse, self._h, lmp, p.size, pp, int(sample_rate))

    def fill_chunk_synthetic(self, n_frames, seed=20260927):
        self._check(self._lib.bp_fill_chunk_synthetic(self._h, int(n_frames), int(seed)))

    def train_resident(self, first_frame, n_frames):
        self._push_hyper()
        self._check(self._lib.bp_train_resident(self._h, int(first_frame), int(n_frames)))

    def train_resident_masked(self, first_frame, n_frames, masks):
        """masks[l], l = 0..numlayers-2: uint8 [n_frames][layersizes[l]] (1 = drop) or None -- parity tests only."""
        P = C.POINTER(C.c_uint8)
        arr = (P * MAXLAYER)()
        keep = []
        for l, m in enumerate(masks):
            if m is not None:
                m = np.ascontiguousarray(m, dtype=np.uint8).reshape(int(n_frames), self.layersizes[l])
                keep.append(m)
                arr[l] = ptr(m)
        self._push_hyper()
        self._check(self._lib.bp_train_resident_masked(self._h, int(first_frame), int(n_frames), arr))

    # ---- gradients without the update (parity tests): bp_grads_resident / bp_read_grads / bp_read_layer_output
    def grads_resident(self, first_frame):
        self._push_hyper()
        self._check(self._lib.bp_grads_resident(self._h, int(first_frame)))

    def grad_floats(self):
        n = C.c_size_t()
        self._check(self._lib.bp_grad_floats(self._h, C.byref(n)))
        return n.value

    def grad_layout(self, layer):
        o, c = C.c_size_t(), C.c_size_t()
        self._check(self._lib.bp_grad_layout(self._h, int(layer), C.byref(o), C.byref(c)))
        return o.value, c.value

    def read_grads(self, padded=False):
        """Per-layer weight / bias gradients of the last bp_grads_resident, unpadded: ([None, G_1 [prev][cur], ...], [None, gb_1, ...]).
        padded: the layers as they lie in the flat buffer (bp_grad_layout), widths rounded up to 64, pad rows and columns included."""
        g = np.empty(self.grad_floats(), np.float32)
        self._check(self._lib.bp_read_grads(self._h, ptr(g), g.size))
        pad = lambda v: (v + 63) & ~63
        gw, gb = [None], [None]
        for l in range(1, self.numlayers):
            off, cnt = self.grad_layout(l)
            lp, lc = pad(self.layersizes[l - 1]), pad(self.layersizes[l])
            assert cnt == lp * lc + lc
            rows, cols = (lp, lc) if padded else (self.layersizes[l - 1], self.layersizes[l])
            gw.append(g[off:off + lp * lc].reshape(lp, lc)[:rows, :cols].copy())
            gb.append(g[off + lp * lc:off + cnt][:cols].copy())
        return gw, gb

    def read_layer_output(self, layer):
        y = np.empty((self.bunchsize, self.layersizes[layer]), np.float32)
        self._check(self._lib.bp_read_layer_output(self._h, int(layer), ptr(y), y.size))
        return y

    # ---- in-library data-parallel exchange (bp_dp_attach, include/bp_c_api.h)
    def dp_attach(self, world, rank, key, transport=0):
        """transport: 0 = the library's peer kernels over hipIpc mappings (reduce-scatter by peer reads), 1 = RCCL reduce-scatter /
        all-gather, 2 = the library's peer kernels in push form (every rank writes its slices into the owners' receive buffers)."""
        self._check(self._lib.bp_dp_attach_ex(self._h, int(world), int(rank), str(key).encode(), int(transport)))

    def dp_peer_info(self, peer):
        """(device ordinal in the peer's process, PCI bus id, transport, acquire mode) of rank `peer`."""
        dev, tr, aq = C.c_int(), C.c_int(), C.c_int()
        buf = C.create_string_buffer(32)
        self._check(self._lib.bp_dp_peer_info(self._h, int(peer), C.byref(dev), buf, 32, C.byref(tr), C.byref(aq)))
        return int(dev.value), buf.value.decode(), int(tr.value), int(aq.value)

    def dp_handoff(self):
        """True: gradient segments are handed to the exchange inside the running weight-gradient launch (tile counters);
        False: event + kernel boundary per group of layers."""
        v = C.c_int()
        self._check(self._lib.bp_dp_handoff(self._h, C.byref(v)))
        return bool(v.value)

    def dp_barrier(self):
        self._check(self._lib.bp_dp_barrier(self._h))

    def dp_allgather_f64(self, value, world):
        mine = (C.c_double * 1)(float(value))
        out = (C.c_double * int(world))()
        self._check(self._lib.bp_dp_allgather(self._h, mine, 8, out))
        return [float(v) for v in out]

    def dp_detach(self):
        self._check(self._lib.bp_dp_detach(self._h))

    def dp_info(self):
        w, r, n = C.c_int(), C.c_int(), C.c_uint()
        self._check(self._lib.bp_dp_info(self._h, C.byref(w), C.byref(r), C.byref(n)))
        return int(w.value), int(r.value), int(n.value)

    def sync(self):
        self._check(self._lib.bp_sync(self._h))

    def last_train_ms(self):
        ms, nb = C.c_float(), C.c_int()
        self._check(self._lib.bp_last_train_ms(self._h, C.byref(ms), C.byref(nb)))
        return float(ms.value), int(nb.value)

    def time_kernel(self, which, iters=50):
        ms = C.c_float()
        self._check(self._lib.bp_time_kernel(self._h, int(which), int(iters), C.byref(ms)))
        return float(ms.value)

    def profile_step(self, first_frame, n_bunches):
        """{class: (avg ms per launch inside the step, launches per step)} -- bp_profile_step."""
        ms = (C.c_float * len(PROF_KINDS))()
        cnt = (C.c_int * len(PROF_KINDS))()
        self._push_hyper()
        self._check(self._lib.bp_profile_step(self._h, int(first_frame), int(n_bunches), ms, cnt))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(PROF_KINDS)}

    def measure_peaks(self):
        a, b = C.c_float(), C.c_float()
        self._check(self._lib.bp_measure_peaks(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def close(self):
        if self._h is not None:
            self._lib.bp_destroy(self._h)       # (releases the handle's open streams too)
            self._h = None


class Stream(object):
    """A streaming session (bp_stream_*): n_chan live feeds enhanced in blocks of any sizes."""

    def __init__(self, owner, s, fea_dim, context, targ_offset, n_chan, packed=False, nat_mode="static", post=False):
        self._g, self._s, self._packed, self._nat_mode, self._post = owner, s, bool(packed), nat_mode, bool(post)
        self.fea_dim, self.context, self.targ_offset, self.n_chan = fea_dim, context, targ_offset, n_chan
        self.look_ahead = context - 1 - targ_offset

    @property
    def packed(self):
        """True for a stream opened in FORWARD_ROWINV: a push places its frames densely and runs the row-invariant forward, whatever
        the handle's mode is by then."""
        return self._packed

    @property
    def nat_mode(self):
        """"static" or "dynamic": the noise-aware block the stream stages -- its handle's mode (set_nat) when it was opened,
        whatever the handle's mode is by then."""
        return self._nat_mode

    @property
    def post(self):
        """True for a stream opened with post-processing on (set_post): it keeps the parameters its handle had then."""
        return self._post

    def push(self, blocks, end=None, out_cap=None):
        """blocks: one 1-D array of new samples per channel (None or empty: none); end: per channel, true closes the channel's
        sentence after these samples.  Returns one float32 array per channel: the samples that became final.  out_cap: size of
        the output buffer in samples (default: everything a push of this size can return)."""
        g = self._g
        if self._s is None or g._h is None:
            g._fail("Stream.push: the stream or its handle is closed")
        if len(blocks) != self.n_chan or (end is not None and len(end) != self.n_chan):
            g._fail("Stream.push: need one block (and one end flag) per channel (%d)" % self.n_chan)
        if out_cap is None:     # what waited (at most max(look-ahead, 5) + 1 frames) and what arrived, rounded up to frames
            out_cap = lambda n: n + self.n_chan * (max(self.look_ahead, 5) + 3) * (self.fea_dim - 1)
        g._push_hyper()
        rc, outs = stream_push(g._lib.bp_stream_push, self._s, self.n_chan, blocks, end, out_cap)
        g._check(rc)
        return outs

    def close(self):
        if self._s is not None and self._g._h is not None:
            self._g._lib.bp_stream_close(self._s)
        self._s = None



def device_count():
    n = C.c_int()
    lib = load_library()
    check(lib, lib.bp_device_count(C.byref(n)))
    return int(n.value)


def device_pci_bus_id(device):
    lib = load_library()
    buf = C.create_string_buffer(32)
    check(lib, lib.bp_device_pci_bus_id(int(device), buf, 32))
    return buf.value.decode()


class Rendezvous(object):
    """bp_rdv_* (include/bp_c_api.h): the host-only rendezvous of the data-parallel ranks; works without a GPU."""

    def __init__(self, key, world, rank, timeout_s=30.0):
        self._lib = load_library()
        self.world, self.rank = int(world), int(rank)
        r, self._r = C.c_void_p(), None
        check(self._lib, self._lib.bp_rdv_open(str(key).encode(), self.world, self.rank, float(timeout_s), C.byref(r)))
        self._r = r

    def barrier(self):
        check(self._lib, self._lib.bp_rdv_barrier(self._r))

    def allgather_f64(self, value):
        mine = (C.c_double * 1)(float(value))
        out = (C.c_double * self.world)()
        check(self._lib, self._lib.bp_rdv_allgather(self._r, mine, 8, out))
        return [float(v) for v in out]

    def close(self):
        if self._r is not None:
            self._lib.bp_rdv_close(self._r)
            self._r = None
