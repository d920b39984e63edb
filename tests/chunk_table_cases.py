"""The host's hop over the `nbytes, nrec` headers of a collated record stream, restated in plain Python (sentences included), and
the streams' building blocks: what tests/test_gpu_chunk_table.py and the far-offset tests judge afq_collated_chunk_table by.
Pure Python / numpy."""
import os
import re

import numpy as np


def hop_tile():
    """kChunkTableTile of csrc/afq_kernels.h: the bytes of the stream the device's hop stages per trip"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alevin-fry_amd", "csrc", "afq_kernels.h")) as f:
        return int(re.search(r"kChunkTableTile = (\d+)", f.read()).group(1))


def host_hop(b, first_chunk, rec_hdr):
    """afq_quantify's hop: (off, nbytes, nrec, first_bc), or the sentence it refuses with.  b: bytes, or anything with len() and
    slices that end with it (Sparse below)"""
    n, p = len(b), first_chunk
    off, nbs, nrs, bcs = [], [], [], []
    while p < n:
        if p + 8 > n:
            return "trailing bytes after the last chunk"
        nb, nr = int.from_bytes(b[p:p + 4], "little"), int.from_bytes(b[p + 4:p + 8], "little")
        if nb < 8 or p + nb > n:
            return "corrupt chunk header"
        if rec_hdr and (nr == 0 or nb < 8 + rec_hdr):
            return f"chunk {len(off)} holds no record"
        off.append(p), nbs.append(nb), nrs.append(nr)
        bcs.append(int.from_bytes(b[p + 12:p + 20].ljust(8, b"\0"), "little"))
        p += nb
    return np.array(off, np.uint64), np.array(nbs, np.uint32), np.array(nrs, np.uint32), np.array(bcs, np.uint64)


def chunk(nb, nr, rng):
    assert nb >= 8
    return int(nb).to_bytes(4, "little") + int(nr).to_bytes(4, "little") + rng.integers(0, 256, nb - 8, dtype=np.uint8).tobytes()


class Sparse:
    """n bytes that are zero but for a few pieces [(offset, bytes)]; a slice of it is bytes and ends with the n bytes, as a slice of
    bytes does.  wrap: every byte address is taken modulo `wrap` first - what a reader sees that drops the high half of its offsets."""

    def __init__(self, n, pieces, wrap=None):
        self.n, self.pieces, self.wrap = n, sorted(pieces), wrap

    def __len__(self):
        return self.n

    def read(self, at, k):
        out = bytearray(k)
        for o, b in self.pieces:
            x, y = max(at, o), min(at + k, o + len(b))
            if x < y:
                out[x - at:y - at] = b[x - o:y - o]
        return bytes(out)

    def __getitem__(self, s):
        a, b, step = s.indices(self.n)
        assert step == 1
        if b <= a:
            return b""
        if self.wrap is None or b <= self.wrap:
            return self.read(a, b - a)
        assert b - a <= 64, "the hop asks for a field at a time"
        return b"".join(self.read(x % self.wrap, 1) for x in range(a, b))
