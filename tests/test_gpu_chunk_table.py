"""GPU tests of afq_collated_chunk_table (csrc/afq_snappy.hip, k_collated_chunk_table): the chunk table of a collated record
stream that lies on the device equals the host's hop over the `nbytes, nrec` headers - restated here in plain Python, sentences
included - at every alignment of the stream, with headers on every side of a tile edge, and on the three refusals."""
import os
import re

import numpy as np
import pytest

from chunk_table_cases import chunk, host_hop   # (one copy, shared with tests/test_gpu_far_offsets.py)
from util import pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "..", "alevin-fry_amd", "csrc", "afq_kernels.h")) as _f:
    TILE = int(re.search(r"kChunkTableTile = (\d+)", _f.read()).group(1))   # bytes of the stream the hop stages per trip


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


def device_table(q, b, first_chunk, rec_hdr, shift):
    import torch

    t = torch.zeros(shift + len(b) + 1, dtype=torch.uint8, device="cuda")   # (one byte of room: an empty stream still has an address)
    if b:
        t[shift:shift + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return q.collated_chunk_table(t.data_ptr() + shift, len(b), first_chunk, rec_hdr)


def check(q, b, first_chunk, rec_hdr, shifts=(0, 1, 2, 3), what=""):
    want = host_hop(b, first_chunk, rec_hdr)
    for shift in shifts:
        if isinstance(want, str):
            with pytest.raises(pkg.AfqError) as e:
                device_table(q, b, first_chunk, rec_hdr, shift)
            assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and str(e.value).endswith(": " + want), (what, shift, str(e.value), want)
        else:
            got = device_table(q, b, first_chunk, rec_hdr, shift)
            for g, w, name in zip(got, want, ("off", "nbytes", "nrec", "first_bc")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (what, shift, name)
    return want


def test_no_chunk_one_chunk_and_one_of_many_tiles(q):
    rng = np.random.default_rng(1)
    pre = rng.integers(0, 256, 37, dtype=np.uint8).tobytes()
    assert len(check(q, pre, 37, 12, what="no chunk")[0]) == 0
    assert len(check(q, b"", 0, 12, what="no byte")[0]) == 0
    assert len(check(q, pre + chunk(20, 1, rng), 37, 12, what="one chunk")[0]) == 1
    assert len(check(q, pre + chunk(5 * TILE + 123, 7, rng), 37, 12, what="one chunk of many tiles")[0]) == 1
    w = check(q, pre + chunk(5 * TILE + 123, 7, rng) + chunk(21, 2, rng) + chunk(TILE, 3, rng) + chunk(33, 4, rng), 37, 12, what="long and short")
    assert list(w[2]) == [7, 2, 3, 4]


def test_the_last_chunk_s_barcode_bytes_end_with_the_buffer(q):
    """records with a 1-byte barcode and a 1-byte UMI: the 8 bytes at chunk + 12 run past the last chunk and the buffer"""
    rng = np.random.default_rng(2)
    for tail in range(14, 21):
        b = chunk(40, 3, rng) + chunk(tail, 1, rng)
        w = check(q, b, 0, 6, what=f"last chunk of {tail} bytes")
        assert int(w[3][1]) >> (8 * (tail - 12)) == 0


def test_headers_on_every_side_of_a_tile_edge(q):
    """the second header stands d bytes from the end of the first tile, d = -28 .. 28: inside the tile, in its halo, behind it"""
    rng = np.random.default_rng(3)
    for first in (0, 3, 50):
        pre = rng.integers(0, 256, first, dtype=np.uint8).tobytes()
        for d in range(-28, 29):
            b = pre + chunk(TILE + d, 5, rng) + chunk(20, 1, rng) + chunk(TILE - 20 + d, 2, rng) + chunk(24, 9, rng) + chunk(2 * TILE - d, 1, rng) + chunk(20, 6, rng)
            w = check(q, b, first, 12, shifts=(d & 3,), what=f"first {first} d {d}")
            assert len(w[0]) == 6


def test_many_small_cells_and_every_shift(q):
    rng = np.random.default_rng(4)
    b = rng.integers(0, 256, 111, dtype=np.uint8).tobytes() + b"".join(chunk(int(nb), int(nb) & 7 or 1, rng) for nb in rng.integers(20, 900, 3000))
    w = check(q, b, 111, 12, what="3000 small cells")
    assert len(w[0]) == 3000
    # more chunks than the first guess of room: a chunk per 4 KiB, 4096 at the least
    b = b"".join(chunk(20, 1, rng) for _ in range(5000))
    assert len(check(q, b, 0, 12, shifts=(1,), what="5000 cells of 20 bytes")[0]) == 5000


@pytest.mark.parametrize("at", [0, 3, 700])
def test_the_three_refusals_at_their_chunk(q, at):
    rng = np.random.default_rng(5)
    good = b"".join(chunk(int(nb), 2, rng) for nb in rng.integers(20, 200, at))
    cases = {
        "trailing": (good + chunk(30, 1, rng) + b"\x14\0\0\0\x01", "trailing bytes after the last chunk"),
        "nbytes below 8": (good + (7).to_bytes(4, "little") + (1).to_bytes(4, "little") + bytes(40), "corrupt chunk header"),
        "nbytes past the end": (good + chunk(30, 1, rng)[:-1], "corrupt chunk header"),
        "nbytes of 4 GiB": (good + b"\xff\xff\xff\xff" + (1).to_bytes(4, "little") + bytes(40), "corrupt chunk header"),
        "no record": (good + chunk(30, 0, rng) + chunk(30, 1, rng), f"chunk {at} holds no record"),
        "shorter than a record": (good + chunk(19, 1, rng) + chunk(30, 1, rng), f"chunk {at} holds no record"),
    }
    for what, (b, sentence) in cases.items():
        assert check(q, b, 0, 12, shifts=(0, 3), what=what) == sentence, what
    # without a record head to ask for (scATAC deduplicate's hop), the last two are tables
    for what in ("no record", "shorter than a record"):
        assert len(check(q, cases[what][0], 0, 0, shifts=(2,), what=what)[0]) == at + 2
    assert len(check(q, good + chunk(30, 1, rng), 0, 12, shifts=(1,), what="the context serves again")[0]) == at + 1
