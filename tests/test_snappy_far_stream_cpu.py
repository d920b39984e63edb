"""Without a device: the streams of snappy_streams.FarStream, whose decoded bytes cross byte 2^32, hold what
tests/test_gpu_snappy_decode.py::test_output_offsets_past_4_gib relies on.  The plan is walked from the stream's own frame headers
(no byte of the 4 GiB is produced): where every far chunk begins, where byte 2^32 falls, the total; and a model of a decoder that
places every chunk at out_off mod 2^32 leaves other bytes in the low region than the stream says."""
import pytest

import snappy_judge as sj
import snappy_streams as ss
from util import pkg

FAR = ss.FAR


def walk(stream):
    """(type, in_off, in_len, ulen) of every data chunk, from the frame headers and the blocks' own lengths"""
    assert stream[:len(sj.STREAM_ID)] == sj.STREAM_ID
    p, out = len(sj.STREAM_ID), []
    while p < len(stream):
        t, n = stream[p], int.from_bytes(stream[p + 1:p + 4], "little")
        assert t in (0, 1) and n >= 4
        out.append((t, p + 8, n - 4, sj._uvarint(stream, p + 8)[0] if t == 0 else n - 4))
        p += 4 + n
    assert p == len(stream)
    return out


@pytest.fixture(scope="module", params=sorted(ss.FAR_STREAMS))
def fs(request):
    return ss.FarStream(request.param)


def test_the_plan_of_the_stream(fs):
    stream = fs.stream()
    pc = pkg.afquant.snappy_decode_limits()["piece_chunks"]
    plan = walk(stream)
    assert 150e6 < len(stream) < 300e6 and len(plan) == fs.n_chunks > 16 * pc
    offs, o = [], 0
    for _, _, _, ulen in plan:
        offs.append(o)
        o += ulen
    assert o == fs.total and FAR < fs.total < FAR + (1 << 20)
    # the groups lie where the builder says, and in the stream where the walk finds them
    for g in ("first", "low", "short filler", "far"):
        for i, off, c in fs.group(g):
            t, in_off, in_len, ulen = plan[i]
            assert offs[i] == off and ulen == len(c.data) and t == (0 if c.compressed else 1) and stream[in_off:in_off + in_len] == c.body, (g, i)
    assert fs.group("first")[0][:2] == (0, 0) and [i for i, _, _ in fs.group("low")] == list(range(1, 1 + ss.FAR_LOW))
    assert len(fs.group("low")) == ss.FAR_LOW and len(fs.group("far")) == ss.FAR_GROUP
    assert all(i > 1 << 16 for i, _, _ in fs.group("far"))
    assert all(u == 65536 for _, _, _, u in plan[1 + ss.FAR_LOW:1 + ss.FAR_LOW + fs.n_fillers]) and offs[1 + ss.FAR_LOW] % 65536 != 0
    # byte 2^32
    si, so, sc = fs.straddler()
    assert so == FAR - fs.before and so + len(sc.data) > FAR
    kind, at, n = fs.elem_at(fs.before)
    if fs.name == "in a literal":
        assert fs.before % 16 != 0 and kind == "lit" and at < fs.before < at + n - 1
    elif fs.name == "in a copy":
        assert kind == "copy" and at < fs.before < at + n - 1, "strictly inside a copy element's destination"
    else:
        assert fs.before == 0 and so == FAR
    assert sum(n for _, n in fs.straddler_elems) == len(sc.data) and sj.decode(sj.STREAM_ID + sc.frame()).data == sc.data
    if sc.compressed:   # the element list is the block's
        lits, copies = [n for k, n in fs.straddler_elems if k == "lit"], [n for k, n in fs.straddler_elems if k == "copy"]
        s = sj.decode(sj.STREAM_ID + sc.frame())
        assert (s.literal_bytes, s.copies) == (sum(lits), len(copies))
    # the twins: low chunk j lies 2^32 below the far chunk j + 1 behind the straddler, with its length and other bytes; the first
    # chunk lies 2^32 below the straddler's bytes from byte 2^32 on
    far = fs.group("far")
    for (li, lo, lc), (fi, fo, fc) in zip(fs.group("low"), far[ss.FAR_STRADDLER + 1:]):
        assert fo - FAR == lo and len(lc.data) == len(fc.data) and (lc.data != fc.data or not fc.data) and lc.compressed == fc.compressed, (li, fi)
    assert len(fs.group("first")[0][2].data) == len(sc.data) - fs.before and fs.group("first")[0][2].data != sc.data[fs.before:]
    assert {len(c.data) for _, _, c in far} >= {0, 1, 40, 4097} and {c.compressed for _, _, c in far} == {True, False}


def test_the_windows_are_the_streams_bytes(fs):
    """FarStream.window against the judge's decode of the stream's ends: the front without the fillers, the back without them"""
    first_filler = next(r for r, (g, _, _) in enumerate(fs.runs) if g == "filler")
    front = sj.decode(sj.STREAM_ID + b"".join(c.frame() for _, c, _ in fs.runs[:first_filler] + [fs.runs[first_filler][:2] + (1,)] * 2)).data
    assert fs.window(0, len(front)) == front
    back = sj.decode(sj.STREAM_ID + b"".join(c.frame() for _, c, _ in fs.runs[first_filler:])).data   # (one filler, then all behind)
    assert fs.window(fs.total - len(back), fs.total + 16) == back + bytes(16)
    assert fs.window(1 << 30, (1 << 30) + 4096) == bytes(4096)
    t = fs.tallies()
    assert t["n_blocks"] == fs.n_chunks and t["n_blocks_stored"] == sum(count for _, c, count in fs.runs if not c.compressed)
    assert t["n_copies"] >= 1024 * fs.n_fillers and t["n_literal_bytes"] >= fs.n_fillers


def test_a_decoder_that_truncates_out_off_changes_the_low_region(fs):
    want, seen = fs.window(0, 1 << 21), fs.window(0, 1 << 21, truncated=True)
    assert want != seen
    # ... in every low chunk that has a byte, and in the first chunk where the straddler's tail is not what is truncated (it begins below 2^32)
    for _, o, c in fs.group("low"):
        assert not c.data or want[o:o + len(c.data)] != seen[o:o + len(c.data)], o
    if fs.before == 0:
        assert want[:4097] != seen[:4097]
    assert fs.window(FAR - (1 << 20), fs.total) != fs.window(FAR - (1 << 20), fs.total, truncated=True), "and the far region misses them"
