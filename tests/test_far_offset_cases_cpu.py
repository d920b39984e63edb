"""Without a device: every placement of tests/far_offset_cases.py puts byte 2^32 where its layout's name says, keeps every piece
inside the buffer, and comes with decoys that the family's judge tells from the original - the statement that a kernel which drops
the high half of an offset cannot pass tests/test_gpu_far_offsets.py.  The same three statements for the chunk-table placements and
the convert placements, further down."""
import pytest

import far_offset_cases as F

FAR = F.FAR


@pytest.fixture(scope="module", params=sorted(F.FAMILIES))
def fam(request):
    f = F.FAMILIES[request.param]
    lim = f.limits() if f.limits else None
    return f, lim, F.placements(f, lim)


def raw(c):
    return c["data"].tobytes() if not isinstance(c["data"], bytes) else c["data"]


def test_every_layout_of_the_family_applies_and_every_piece_lies_inside_the_buffer(fam):
    f, lim, pl = fam
    assert {layout for _, layout, _, _, _ in pl} == set(f.layouts)
    assert "widths" in {name for name, *_ in pl}
    for name, layout, pad, c, (pieces, new_off, n_bytes) in pl:
        assert n_bytes == FAR + (1 << 21) and len(new_off) == len(c["off"])
        assert all(0 <= o and o + len(b) <= n_bytes - 16 for o, b in pieces), (f.name, name, layout)
        assert sum(len(b) for _, b in pieces) < 1 << 20   # (a few pieces, never gigabytes of Python bytes)
        walked = F.walk(raw(c), c["off"], *f.layout(c))
        real = dict((o, b) for o, b in pieces[:len(new_off)])
        assert [real[int(o)] for o in new_off] == F.chunk_bytes(raw(c), c["off"], walked), "the chunks' contents are unchanged"
        n_decoys = sum(1 for o, (nb, _) in zip(new_off, walked) if int(o) + nb > FAR)
        assert len(pieces) == len(new_off) + n_decoys and n_decoys >= 1
        for (o, b), (ro, rb) in zip(pieces[len(new_off):], [(int(o), real[int(o)]) for o, (nb, _) in zip(new_off, walked) if int(o) + nb > FAR]):
            skip = max(0, FAR - ro)
            assert o == ro + skip - FAR and len(b) == len(rb) - skip and (b != rb[skip:] or not any(w[1] for w in F.walk(rb, [0], *f.layout(c))))


def test_byte_two_to_the_32_lies_where_the_layouts_name_says(fam):
    f, lim, pl = fam
    for name, layout, pad, c, (pieces, new_off, _) in pl:
        fields, A = f.layout(c)
        walked = F.walk(raw(c), c["off"], fields, A)
        at = F.where(raw(c), c["off"], new_off, fields, A)
        far = F.far_chunks(new_off)
        what = (f.name, name, layout, at)
        if layout == "low-high":
            assert at is None and far == list(range(1, len(new_off))) and int(new_off[0]) == pad and int(new_off[1]) == FAR + F.GAP + pad, what
        elif layout == "descending":
            assert at is None and far == [i for i in range(len(new_off)) if i != 1] and int(new_off[1]) == pad and int(new_off[0]) > FAR, what
        elif layout == "start-on":
            ci = at[0]
            assert at[1:] == (None, "nbytes", 0) and ci >= 1 and int(new_off[ci - 1]) + walked[ci - 1][0] == FAR and far == list(range(ci, len(new_off))), what
        elif layout == "straddle-head":
            ci, r, field, k = at
            assert (field, k) == ("na", 2) and 0 < r < len(walked[ci][1]) - 1, what
        elif layout == "straddle-list":
            ci, r, field, k = at
            na = walked[ci][1][r][1]
            assert field[0] == "aln" and na > 64 and 64 <= field[1] < na and 0 < k, what
        else:
            ci, r, field, k = at
            ts = F.tile_starts(walked[ci][1], lim["parse_tile"])
            assert len(ts) >= 3, what
            j = FAR - int(new_off[ci])
            if layout == "tile-first":
                assert (field, k) == ("na", 0) and j == ts[1] == walked[ci][1][r][0], what
            else:
                assert j == ts[1] + lim["parse_tile"] - 1 and j < ts[2], what


def test_the_judge_tells_the_decoys_from_the_original(fam):
    f, lim, pl = fam
    wants, lines = {}, []
    for name, layout, pad, c, (pieces, new_off, _) in pl:
        fields, A = f.layout(c)
        seen = F.decoy_view(raw(c), c["off"], new_off, fields, A, f.aln_flip)
        assert seen != raw(c) and len(seen) == len(raw(c))
        for ori in f.oris:
            if (name, ori) not in wants:
                wants[(name, ori)] = F.canon(f.want(c, ori, lim))
                assert F.canon(f.from_bytes(c, raw(c), ori, lim)) == wants[(name, ori)], (f.name, name, ori, "the bytes read back do not say what the case says")
            differs = F.canon(f.from_bytes(c, seen, ori, lim)) != wants[(name, ori)]
            lines.append(f"{f.name} / {name} / {layout} pad {pad} / {ori or '-'}: judge(decoys) {'!=' if differs else '=='} judge(original)")
            assert differs, lines[-1]
    print("\n".join(lines))   # (shown under -s: one line per family, case, layout and orientation)


# ------------------------------------------------------------------------------------------------------------------ the chunk table
import chunk_table_cases as T


@pytest.fixture(scope="module", params=F.CT_HEADERS_AT, ids=lambda at: f"header at 2^32 - {FAR - at}")
def ct(request):
    return F.chunk_table_placement(request.param, T.hop_tile())


def test_chunk_table_placement_puts_byte_two_to_the_32_where_it_says(ct):
    at, off, nb = ct["at"], ct["off"], ct["nbytes"]
    assert F.chunk_table_where(ct) == F.CT_WHERE[at] and off[ct["k_at"]] == at
    assert (FAR in off) == (at == FAR - 20), "FAR - 20: a chunk of 20 bytes, and a header on byte 2^32"
    assert off[0] == F.CT_FIRST == 37 and off[1] == off[0] + nb[0] and abs(nb[0] - (1 << 31)) < 1 << 20 and abs(nb[1] - (1 << 31)) < 1 << 20
    assert all(20 <= x <= 900 for x in nb[2:ct["k_at"]]) and sum(1 for o in off if o > FAR) >= 300 and max(nb[2:]) > T.hop_tile()
    assert nb[-1] == 15 and ct["n"] == off[-1] + 15 and ct["n_whole"] == off[-1] and ct["n"] + F.CT_GUARD + 3 <= F.N_BYTES
    pieces = sorted(ct["pieces"])
    assert all(a + len(x) <= b for (a, x), (b, _) in zip(pieces, pieces[1:])) and sum(len(b) for _, b in pieces) < 1 << 20
    assert pieces[-1] == (ct["n"], b"\xff" * F.CT_GUARD), "what stands behind the stream is not zero"


def test_chunk_table_wanted_tables_and_refusals(ct):
    """the hop over the sparse view is the table the builder laid out; the stream's ends give the three refusals behind byte 2^32"""
    n_chunks = len(ct["off"])
    for n, rec_hdr, k in ((ct["n"], 6, n_chunks), (ct["n"], 0, n_chunks), (ct["n_whole"], 12, n_chunks - 1)):
        off, nbs, nrs, bcs = T.host_hop(F.chunk_table_view(ct, n), F.CT_FIRST, rec_hdr)
        assert off.tolist() == ct["off"][:k] and nbs.tolist() == ct["nbytes"][:k] and nrs.tolist() == ct["nrec"][:k]
        assert len(set(bcs.tolist())) > k - 5 and (k < n_chunks or int(bcs[-1]) >> 24 == 0), "15 bytes: three of barcode, and zeros not the guard"
    for rec_hdr in (12, 0):
        assert T.host_hop(F.chunk_table_view(ct, ct["n_whole"] + 5), F.CT_FIRST, rec_hdr) == "trailing bytes after the last chunk"
        assert T.host_hop(F.chunk_table_view(ct, ct["n"] - 1), F.CT_FIRST, rec_hdr) == "corrupt chunk header"
    assert T.host_hop(F.chunk_table_view(ct), F.CT_FIRST, 12) == f"chunk {n_chunks - 1} holds no record"
    nr = F.chunk_table_placement(ct["at"], T.hop_tile(), no_record=True)
    K = nr["k_at"] + 2
    assert nr["off"][K] > FAR and T.host_hop(F.chunk_table_view(nr, nr["n_whole"]), F.CT_FIRST, 12) == f"chunk {K} holds no record"
    assert len(T.host_hop(F.chunk_table_view(nr, nr["n_whole"]), F.CT_FIRST, 0)[0]) == n_chunks - 1


def test_a_hop_that_truncates_its_addresses_gives_another_table(ct):
    for n, rec_hdr in ((ct["n"], 6), (ct["n"], 0), (ct["n_whole"], 12)):
        want = T.host_hop(F.chunk_table_view(ct, n), F.CT_FIRST, rec_hdr)
        seen = T.host_hop(F.chunk_table_view(ct, n, truncated=True), F.CT_FIRST, rec_hdr)
        k = ct["k_at"]
        if isinstance(seen, str):
            print(f"header at 2^32 - {FAR - ct['at']}, rec_hdr {rec_hdr}: the truncated hop refuses ({seen})")
            continue
        assert any(a[:k + 2].tolist() != b[:k + 2].tolist() for a, b in zip(want[1:], seen[1:])), "by the chunk behind the header at the latest"
    # and whatever it does, every chunk whose fields lie behind byte 2^32 reads other fields there
    v, t = F.chunk_table_view(ct), F.chunk_table_view(ct, truncated=True)
    for p in ct["off"][2:]:
        if p >= FAR:
            assert v[p:p + 4] != t[p:p + 4] and v[p + 4:p + 8] != t[p + 4:p + 8] and v[p + 12:p + 20] != t[p + 12:p + 20], p - FAR


# ------------------------------------------------------------------------------------------------------------------ convert
import bam_cases as B
import convert_judge as J
from util import pkg

BAM_WHERE = {"block_size": "block_size", "l_read_name": "l_read_name", "flag": "flag", "name": "name", "CR": ("CR", "value"), "UR": ("UR", "value"), "AS": ("AS", "value"),
             "start-on": "block_size"}


@pytest.fixture(scope="module", params=F.BAM_PLACEMENTS)
def bam(request):
    lim = pkg.convert_limits()
    return F.bam_placement(request.param, lim), lim


def state(records, fb, lim):
    return J.stated(records, fb, n_ref=F.BAM_N_REF, lane_alns=lim["lane_alns"], bw=F.BAM_BW, uw=F.BAM_UW)


def test_bam_placement_is_a_record_stream_with_byte_two_to_the_32_where_it_says(bam):
    pl, lim = bam
    recs, offs, n = pl["records"], pl["offs"], pl["n_bytes"]
    view = T.Sparse(n, pl["pieces"])
    p, walked = 0, []   # the block_size chain over the sparse bytes finds every record, the fillers included, and ends with the stream
    while p < n:
        walked.append(p)
        p += 4 + int.from_bytes(view[p:p + 4], "little")
    assert p == n and walked == offs and len(offs) == len(recs) and FAR < n < FAR + (1 << 20)
    f1, f2 = pl["fillers"]
    for f in (f1, f2):
        assert view[offs[f]:offs[f] + 36] == F.bam_filler_bytes(offs[f + 1] - offs[f] - 4) and abs(offs[f + 1] - offs[f] - (1 << 31)) < 1 << 20
        assert view[offs[f] + 36:offs[f] + 4096] == bytes(4060) and recs[f]["flag"] == 0x4
    spans = pl["span_off"]
    assert spans[0] == 0 and spans == sorted(set(spans)) and set(spans) <= set(offs) and {offs[f1], offs[f2], offs[f2 + 1]} <= set(spans) and sum(s > FAR for s in spans) >= 2
    assert spans[spans.index(offs[f1]) + 1] == offs[f2] and spans[spans.index(offs[f2]) + 1] == offs[f2 + 1], "a filler is a span of its own"
    for i, r in enumerate(recs):
        if i not in (f1, f2):
            assert view[offs[i]:offs[i] + len(B.record_bytes(r))] == B.record_bytes(r), i
    # byte 2^32
    t, where = pl["target"], pl["where"]
    k = FAR - offs[t]
    if where == "run-across":
        assert t == pl["high0"] and k == -5 and [r["name"] for r in recs[f1 - 1:f1] + recs[t:t + 3]] == ["across", "across", "across", "a"]
        assert offs[f1 - 1] < 1 << 20 and recs[f1 - 1].get("flag", 0) & 0x804 == 0
    else:
        assert 0 <= k < len(B.record_bytes(recs[t])) and F.bam_field_at(recs[t], k) == BAM_WHERE[where], (where, k)
        assert where != "start-on" or (k == 0 and FAR in spans)
        assert recs[t - 1]["name"] != recs[t]["name"], "the target is a run's head: its CR and UR are read"
    # the decoys: 2^32 below, the same sizes, no character of the name, no base, not the refID, not the AS
    assert len(pl["decoyed"]) >= 30
    for j, i in enumerate(pl["decoyed"]):
        d, r = recs[pl["n_pad"] + j], recs[i]
        assert offs[pl["n_pad"] + j] == offs[i] - FAR and len(B.record_bytes(d)) == len(B.record_bytes(r)) and d["ref"] != r["ref"]
        assert all(a != b for a, b in zip(d["name"], r["name"]))
        for (tag, ty, dv), (_, _, rv) in zip(d["aux"], r["aux"]):
            if tag in ("CR", "UR"):
                assert len(dv) == len(rv) and all(a != b for a, b in zip(dv, rv))
            elif tag == "AS":
                assert dv != rv
    assert all(rr.get("flag", 0) & 0x4 for rr in recs[:pl["n_pad"]])
    assert sum(len(b) for _, b in pl["pieces"]) < 1 << 20


def test_bam_judge_does_not_depend_on_a_dropped_record_s_length_and_tells_the_truncated_view(bam):
    pl, lim = bam
    f1, f2 = pl["fillers"]
    for fb in (False, True):
        want = state(pl["records"], fb, lim)
        for n in (64, 4000):
            other = list(pl["records"])
            other[f1], other[f2] = B.filler(n), B.filler(2 * n)
            assert state(other, fb, lim) == want
        assert want["stats"]["n_records"] == len(pl["records"]) and want["stats"]["n_dropped_by_flag"] >= 2 and want["stats"]["n_runs_written"] > 50
        seen = state(F.bam_truncated_records(pl), fb, lim)
        assert seen["bytes"] != want["bytes"], (pl["where"], fb)


def test_bam_refusals_name_a_record_behind_byte_two_to_the_32_and_stay_inside_the_stream():
    lim = pkg.convert_limits()
    rs = F.bam_refusals(lim)
    assert len(rs) == 2
    for what, pl, index in rs:
        assert index == len(pl["records"]) - 1 and pl["offs"][index] > FAR and pl["span_off"][-1] <= pl["offs"][index]
        raw = B.record_bytes(pl["records"][index])
        assert pl["offs"][index] + len(raw) == pl["n_bytes"], "the stream ends with the record's own bytes"
        bs = int.from_bytes(raw[:4], "little")
        assert (bs == 4000 and 4 + bs > len(raw)) if "block_size" in what else (4 + bs == len(raw) and raw.endswith(b"XY"))
        state(pl["records"][:index], False, lim)   # every record in front is in order
