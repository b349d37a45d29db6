"""NumPy / plain Python restatement of the streaming contract of bp_stream_push (include/bp_c_api.h): what a
channel has produced after `received` samples of its sentence.  Written from the formulas, not from csrc/bp_stream.hip."""
import numpy as np


def counts(fea_dim, context, targ_offset, nat, received, ended):
    """(frames_in, frames_out, samples_out)."""
    hop = fea_dim - 1
    la = context - 1 - targ_offset
    if received == 0:
        return 0, 0, 0
    T = (received - 1) // hop + 2
    frames_in = T if ended else received // hop          # frame t needs the real samples [(t-1) hop, (t+1) hop)
    known = (not nat) or ended or frames_in >= 6         # the noise-aware row: 6 frames, or the offline clamp at the end
    if not known:
        frames_out = 0
    else:
        frames_out = T if ended else max(0, frames_in - la)
    samples_out = received if ended else max(0, frames_out - 1) * hop
    return frames_in, frames_out, samples_out


def ragged_schedule(rng, n, hop, zero_share=0.2):
    """Block sizes that sum to n: zeros, single samples, sizes around the hop and larger ones."""
    out = []
    while n > 0:
        k = rng.integers(0, 5)
        b = 0 if rng.random() < zero_share else int([1, rng.integers(1, hop), hop, rng.integers(hop, 3 * hop + 2), rng.integers(1, 9 * hop)][k])
        b = min(b, n)
        out.append(b)
        n -= b
    return out
