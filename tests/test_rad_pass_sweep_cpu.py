"""Without a device: what the fixed seeds of tests/rad_pass_sweep.py reach together, family by family - every width value, every
alignment of a chunk start, a chunk of three tiles, an empty chunk between others, a long record at batch index 64 or beyond of its
tile, for the collates a kept long record with position bytes and fitting words on both sides of index 64, a record of every fate -
and that the family's judge takes every draw.  A witness that fails asks for other seeds, not for another witness."""
import time

import pytest

import far_offset_cases as F
import rad_pass_sweep as S


@pytest.fixture(scope="module", params=S.FAMILIES)
def drawn(request):
    fam = request.param
    lim = S.LIMITS[fam]()
    return fam, lim, [S.draw(fam, seed, lim) for seed in S.SEEDS[fam]]


def layout(fam, c):
    return F.FAMILIES[fam].layout(c)


def raw(c):
    return c["data"] if isinstance(c["data"], bytes) else bytes(c["data"])


def tiles_of(fam, c, lim):
    """per chunk: [(index of the chunk's record, its place in its tile's batch)]"""
    fields, A = layout(fam, c)
    out = []
    for nb, recs in F.walk(raw(c), c["off"], fields, A):
        ts = F.tile_starts(recs, lim["parse_tile"])
        first = [next(i for i, (q, _) in enumerate(recs) if q == p) for p in ts]
        out.append((len(ts), [(i, i - max(f for f in first if f <= i)) for i in range(len(recs))]))
    return out


def test_eight_seeds_a_family_and_draws_that_repeat(drawn):
    fam, lim, cases = drawn
    assert len(S.SEEDS[fam]) == len(set(S.SEEDS[fam])) == 8
    again = S.draw(fam, S.SEEDS[fam][0], lim)
    assert raw(again) == raw(cases[0]) and again["off"].tolist() == cases[0]["off"].tolist()
    assert len({raw(c) for c in cases}) == 8


def test_the_draws_reach_every_width_alignment_and_chunk_shape(drawn):
    fam, lim, cases = drawn
    widths = {k: {c[k] for c in cases} for k in cases[0] if k.endswith("_bytes")}
    if fam in ("gpl", "collate"):
        assert widths == {"bc_bytes": set(S.G.WIDTHS), "umi_bytes": set(S.G.WIDTHS), "pos_bytes": set(S.POS_BYTES[fam])}, widths
    elif fam in ("gpl multi", "collate multi"):
        assert widths == {"b0_bytes": set(S.MC.B_WIDTHS), "b1_bytes": set(S.MC.B_WIDTHS), "umi_bytes": set(S.MC.U_WIDTHS), "pos_bytes": set(S.POS_BYTES[fam])}, widths
    else:
        assert widths == {"bc_bytes": set(S.ATAC_WIDTHS)}, widths
    assert {int(o) % 4 for c in cases for o in c["off"]} == {0, 1, 2, 3}
    assert {int(c["off"][0]) for c in cases} == {0, 1, 2, 3}   # the pad bytes
    assert {len(c["off"]) for c in cases} >= {1, 6} and all(1 <= len(c["off"]) <= 6 for c in cases)
    nrec = [[len(r) for r in c["chunks"]] for c in cases]
    assert any(n[i] == 0 and any(n[:i]) and any(n[i + 1:]) for n in nrec for i in range(len(n))), "no empty chunk between non-empty ones"
    assert sum(1 for n in nrec if n.count(0) > 1) == 0   # (one chunk of a draw may be empty)
    assert any(nt >= 3 for c in cases for nt, _ in tiles_of(fam, c, lim)), "no chunk of three tiles"
    assert max(len(raw(c)) for c in cases) <= 6 * (3 * lim["parse_tile"] + lim["parse_tile"] // 2 + 3000)


def test_the_draws_reach_a_long_record_late_in_its_batch(drawn):
    fam, lim, cases = drawn
    hit = 0
    for c in cases:
        for recs, (_, places) in zip(c["chunks"], tiles_of(fam, c, lim)):
            for i, at in places:
                na = len(recs[i][-1])
                hit += at >= 64 and (na > lim["lane_alns"] if fam in S.RNA else na == 1)   # (ATAC: a record the pass keeps)
    assert hit >= 2, hit
    if fam in S.RNA:
        nas = {len(r[-1]) for c in cases for recs in c["chunks"] for r in recs}
        L = lim["lane_alns"]
        assert nas >= {0, 1, 2, 3, 4, 5, L - 1, L, L + 1, L + 2} and any(64 < n for n in nas) and max(nas) <= 200, sorted(nas)
    else:
        assert {len(r[-1]) for c in cases for recs in c["chunks"] for r in recs} == {0, 1, 2, 5}


def fits(alns, ori):
    return [j for j, (_, fw) in enumerate(alns) if ori == "both" or fw == (ori == "fw")]


def fate(fam, c, r, ori):
    """what becomes of record r of case c, said from the case's own tables"""
    if fam in S.RNA and not (ori == "both" or fits(r[-1], ori)):
        return "incompatible"
    if fam == "gpl":
        return "counted"
    if fam == "gpl multi":
        return "routed" if r[0] in c["entries"] else "unrouted"
    if fam == "collate":
        return "uncorrected" if r[0] not in c["corrections"] else ("kept" if c["corrections"][r[0]] == r[0] else "corrected")
    if fam == "collate multi":
        if r[0] not in c["sample_table"]:
            return "unrouted"
        s = c["sample_table"][r[0]]
        return "uncorrected" if (s, r[1]) not in c["cell_table"] else ("kept" if c["cell_table"][(s, r[1])] == r[1] else "corrected")
    if fam == "atac gpl":
        return ("unmapped", "binned", "multimapped")[min(len(r[1]), 2)]
    if len(r[1]) != 1:
        return ("unmapped", "", "multimapped")[min(len(r[1]), 2)]
    if fam == "atac sort":
        m = dict(zip(c["obs"].tolist(), c["cor"].tolist()))
        return "uncorrected" if r[0] not in m else ("kept" if m[r[0]] == r[0] else "corrected")
    return "uncorrected" if r[0] not in c["corrections"] else ("kept" if c["corrections"][r[0]] == r[0] else "corrected")


def in_tables(fam, c, r):
    if fam == "gpl multi":
        return r[0] in c["entries"]
    if fam == "collate multi":
        return r[0] in c["sample_table"]
    if fam == "atac sort":
        return r[0] in set(c["obs"].tolist())
    return r[0] in c["corrections"]


FATES = {"gpl": {"counted", "incompatible"}, "gpl multi": {"routed", "unrouted", "incompatible"}, "atac gpl": {"unmapped", "binned", "multimapped"},
         "collate": {"kept", "corrected", "uncorrected", "incompatible"}, "collate multi": {"kept", "corrected", "unrouted", "uncorrected", "incompatible"},
         "atac sort": {"kept", "corrected", "uncorrected", "unmapped", "multimapped"}, "atac collate": {"kept", "corrected", "uncorrected", "unmapped", "multimapped"}}


def test_the_draws_reach_every_fate_and_the_collates_a_kept_long_record_with_positions(drawn):
    fam, lim, cases = drawn
    for ori in S.ORIS[fam]:
        if ori == "both":
            continue
        seen = {fate(fam, c, r, ori) for c in cases for recs in c["chunks"] for r in recs}
        assert seen == FATES[fam], (ori, seen)
        # every fate on a record of more alignments than a lane takes, and the barcodes 0 and all-ones on records
        if fam in S.RNA:
            long_seen = {fate(fam, c, r, ori) for c in cases for recs in c["chunks"] for r in recs if len(r[-1]) > lim["lane_alns"]}
            assert long_seen == FATES[fam], (ori, long_seen)
        if fam in ("collate", "collate multi"):
            hit = 0
            for c in cases:
                for recs in c["chunks"]:
                    for r in recs:
                        f = fits(r[-1], ori)
                        hit += c["pos_bytes"] > 0 and len(r[-1]) > 64 and fate(fam, c, r, ori) in ("kept", "corrected") and len(f) >= 2 and f[0] < 64 <= f[-1]
            assert hit >= 2, (ori, hit)
    key = "b1_bytes" if fam in ("gpl multi", "collate multi") else "bc_bytes"
    at = 1 if fam in ("gpl multi", "collate multi") else 0
    assert all(any(r[at] == v for recs in c["chunks"] for r in recs) for c in cases if sum(map(len, c["chunks"])) > 200 for v in (0, (1 << (8 * c[key])) - 1))
    if fam not in ("gpl", "atac gpl"):   # about a fifth of the records on barcodes outside the tables, and what the planner leaves out
        out = [sum(not in_tables(fam, c, r) for recs in c["chunks"] for r in recs) / max(1, sum(map(len, c["chunks"]))) for c in cases]
        assert 0.1 < sum(out) / len(out) < 0.6, out


def test_the_judge_takes_every_draw(drawn):
    fam, lim, cases = drawn
    worst = 0.0
    for c in cases:
        for ori in S.ORIS[fam]:
            t0 = time.perf_counter()
            w = S.want(fam, c, ori, lim)
            worst = max(worst, time.perf_counter() - t0)
            assert w is not None
        # the bytes tile, chunk by chunk, as the family's layout says
        fields, A = layout(fam, c)
        assert [len(recs) for _, recs in F.walk(raw(c), c["off"], fields, A)] == [len(r) for r in c["chunks"]]
    print(f"{fam}: slowest want() {worst:.3f} s")   # (the figures of rad_pass_sweep's docstring; shown under -s)
