"""CPU-only: what the one-call decodes of LZ4Stream buffers and wrapped messages rely on, under the SIMT emulator with the REAL decoder
kernels: a known-size decode answers a row of length 0 and capacity 0 -- a table row past the count, or one clipped at dst_cap -- with a
negative result and touches no byte, in every mapping the library dispatches to, and the rows around it decode as usual."""
import numpy as np
import pytest

import emu_helpers as emu

# the wavefront decoder; lane generation 4 in the default configuration, plain and persistent (one and three wavefronts); workgroups
# of four wavefronts with dual ring stores and with wrapped rows
MAPPINGS = {"wave-per-block": {}, "l4c59192": dict(lane=59192, gen=4), "l4p1": dict(lane=1, gen=5), "l4p3": dict(lane=3, gen=5),
            "l4w1": dict(lane=1, gen=6), "l4w2": dict(lane=2, gen=6)}


@pytest.mark.parametrize("mapping", list(MAPPINGS), ids=list(MAPPINGS))
def test_empty_rows_fail_and_touch_nothing(oracle, mapping):
    good = oracle.gen(2, 5, 3, 1, 3000)[0][:3000]
    comp = oracle.compress(good)
    empty = np.zeros(0, np.uint8)
    for at, n in ((0, 1), (3, 7), (66, 70), (69, 70)):                     # the good block first, among, in a second wavefront, last
        comps = [comp if i == at else empty for i in range(n)]
        sizes = [good.size if i == at else 0 for i in range(n)]
        res, dst = emu.decode(comps, sizes, known=True, **MAPPINGS[mapping])
        for i in range(n):
            if i == at:
                assert res[i] == comp.size and np.array_equal(dst[i, :good.size], good), (mapping, n, i, res[i])
                assert (dst[i, good.size:] == 0xA5).all(), (mapping, n, i)
            else:
                assert res[i] < 0, (mapping, n, i, res[i])
                assert (dst[i] == 0xA5).all(), (mapping, n, i, "an empty row's slot was written")
    # a batch of empty rows alone
    res, dst = emu.decode([empty] * 5, [0] * 5, known=True, **MAPPINGS[mapping])
    assert (res < 0).all() and (dst == 0xA5).all(), (mapping, res.tolist())
