"""The synchronisation index of the JPEG test cases, restated on the host from tests/
jpeg_case.py's sequential decoder: the state at the first symbol at or after every multiple
of SUB_BITS, and the blocks each subsequence completes when decoded from its state.  Shared
by the pack format test and the device index tests; computed once per case and process."""
import numpy as np

import jpeg_case as jc

from monodepth2_amd.jpeg_ops import pack_index

_INDEX = {}


def restated(name):
    """(states, first_blocks) of case `name`: python ints, one per subsequence."""
    if name not in _INDEX:
        s = jc.parsed(name)
        _, done, boundaries, E = jc.sequential_coefficients(s)
        assert done == E.total_blocks and len(boundaries) == E.nsub, name
        states = [(p << 16) | (b << 8) | k for p, b, k in boundaries]
        first, g = [], 0
        for i in range(E.nsub):
            first.append(g)
            g += E.decode(boundaries[i], jc.SUB_BITS * (i + 1))[1]
        assert g == E.total_blocks, (name, g, E.total_blocks)
        _INDEX[name] = (states, first)
    return _INDEX[name]


def restated_bytes(name) -> np.ndarray:
    """The restated index in the stored layout (jpeg_ops.pack_index)."""
    out = pack_index(*restated(name))
    out.setflags(write=False)
    return out
