"""Plain Python restatement of the counts of a log-MMSE stream (bp_lmstream_counts, include/bp_c_api.h): what a
channel has produced after `received` samples of its sentence.  Written from the formulas, not from csrc/bp_classic.hip."""


def counts(fea_dim, init_frames, received, ended):
    """(frames_in, frames_out, samples_out)."""
    hop = fea_dim - 1
    if received == 0:
        return 0, 0, 0
    T = (received - 1) // hop + 2
    frames_in = T if ended else received // hop          # frame t needs the real samples [(t-1) hop, (t+1) hop)
    known = ended or frames_in >= init_frames            # the noise start: the first min(init_frames, T) frames
    frames_out = 0 if not known else (T if ended else frames_in)
    samples_out = received if ended else max(0, frames_out - 1) * hop
    return frames_in, frames_out, samples_out
