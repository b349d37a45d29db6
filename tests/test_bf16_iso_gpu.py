"""Each bf16 step kernel alone on known operands, against float64 at half-ulp bars (-m gpu).  tests/bf16_iso.py has the cases, the
constructions, the references and the bars; tests/test_bf16_iso_host.py proves on the CPU that every observation shows the hidden
tensor it claims to show and that the bars see wrong kernels.  A failure names the tensor and the worst 64 x 64 block; every
measured error / bar ratio goes to the parity record, and profiles/bf16_iso_parity_numbers.json holds those of the committed run."""
import numpy as np
import pytest

import bf16_iso as I
from test_dispatch_gpu import worst_block

pytestmark = pytest.mark.gpu


class Handle(object):
    """What bf16_iso.run_case asks of a device, on a bf16 handle."""

    def __init__(self, pkg, ls, B, act, out, W, b):
        kw = dict(activation=act, compute_dtype=1, max_chunk_frames=B)
        if out is not None:
            kw.update(output_activation=1, output_linear_cols=out[0], output_loss=out[1])
        self.g = pkg.BP_GPU(1, len(ls), ls, B, I.LR, I.MOM, I.WC, W, b, **kw)
        self.B = B

    def forward(self, x):
        return self.g.forward(x)

    def grads(self, x, t):
        self.g.upload_chunk(x, t)
        self.g.grads_resident(0)
        return self.g.read_grads(padded=True)

    def train(self, x, t):
        self.g.train(self.B, x, t)
        return self.g.get_weights() + self.g.get_deltas()

    def close(self):
        self.g.close()


@pytest.mark.parametrize("cid", [c.id for c in I.CASES])
def test_kernel_alone(pkg, parity_record, cid):
    c = I.BY_ID[cid]
    res = I.run_case(c, lambda *a: Handle(pkg, *a))
    ratios, fails = {}, []
    for ch in res.checks:
        ratios[ch.name] = r = I.ratio_of(ch)[0]
        if not r <= 1.0:
            got, ref = np.atleast_2d(ch.got), np.atleast_2d(ch.ref)
            fails.append("%s: error / bar %.3g%s%s; %s" % (ch.name, r, " (bit for bit)" if ch.bar is None else "",
                                                          " (not all bf16 numbers)" if ch.bf16 and not I.is_bf16(ch.got) else "",
                                                          worst_block(got, ref) if got.shape == ref.shape else "shapes %s, %s" % (got.shape, ref.shape)))
    print(cid, c.kernel, "error / bar:", ratios, res.figures)
    parity_record(bf16_iso={"kernel": c.kernel, "error_over_bar": ratios, "figures": res.figures})
    assert not fails, (cid, c.kernel, fails)
