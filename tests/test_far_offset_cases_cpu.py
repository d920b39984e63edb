"""Without a device: every placement of tests/far_offset_cases.py puts byte 2^32 where its layout's name says, keeps every piece
inside the buffer, and comes with decoys that the family's judge tells from the original - the statement that a kernel which drops
the high half of an offset cannot pass tests/test_gpu_far_offsets.py."""
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
