"""The dense rule rounds of k_resolve_hash, against the oracle (bit-exact).  After the insert phase the bucket's UMIs - the
slots its lanes claimed - are numbered 0 .. U-1 and lane l of rule round r resolves owner 64 r + l, so the kernel's paths change
at U = 64, 128, 192 whatever the number of keys n is.  Each case is one cell of 257 .. 512 single-ref reads, which the planner
gives two buckets (256 << lg >= n_ref); the UMIs are 32-bit and are picked with a numpy restatement of bucket_of (afq_common.h:
for them the bucket is the top bit of umi * 0x9E3779B1 mod 2^32), so that bucket 0 holds exactly the n keys and U UMIs the case
is about and bucket 1 the padding.  small_thresh = 0.  Every case asserts that nothing was diverted: a bucket that reached the
sort path proves nothing about the table."""
import numpy as np
import pytest

from util import assert_same_result, pkg

rad = pkg.rad

N_TXP = 40
BOUNDARY_U = [1, 63, 64, 65, 127, 128, 129, 192, 193, 256]


def bucket_of_lg1(umi):
    """bucket_of(umi, 1) of afq_common.h for UMIs under 2^32"""
    return ((np.asarray(umi, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(31)


def _umi_pools():
    rng = np.random.default_rng(1201)
    cand = np.unique(rng.integers(1, 0xFFFFFFFE, size=4096, dtype=np.uint64))
    cand = cand[rng.permutation(len(cand))]
    b = bucket_of_lg1(cand)
    return [int(u) for u in cand[b == 0]], [int(u) for u in cand[b == 1]]


POOL0, POOL1 = _umi_pools()


def _genes(i):
    """two refs of distinct genes (identity map, and ref // 2 of the USA map) for UMI i"""
    g1 = (7 * i) % N_TXP
    return g1, (g1 + 2 + i % 5) % N_TXP


def _pad(n0):
    """bucket 1: single-read UMIs that bring the cell to 257 reads at least (two buckets), 24 at least"""
    return [(POOL1[i], [(3 * i) % N_TXP]) for i in range(max(257 - n0, 24))]


def _finish(first, rest, order, seed):
    """bucket-0 reads from the first read of every UMI and the further ones, in one of three input orders, plus the padding"""
    rng = np.random.default_rng(seed)
    if order == "owners-first":
        reads = first + rest
    elif order == "owners-last":
        reads = rest + first
    else:
        reads = first + rest
        reads = [reads[i] for i in rng.permutation(len(reads))]
    pad = _pad(len(reads))
    at = sorted(int(x) for x in rng.integers(0, len(reads) + 1, size=len(pad)))   # the padding in between, order kept
    out, k = [], 0
    for i, r in enumerate(reads + [None]):
        while k < len(pad) and at[k] == i:
            out.append(pad[k])
            k += 1
        if r is not None:
            out.append(r)
    return out


def build_boundary(U, n, order="shuffled"):
    """U UMIs, n reads in bucket 0.  The n - U further reads go round the first UMIs, two or three to each: to every third UMI
    repeats of its gene, to the next a second gene and the first in turn (a tie after an odd number, else the first gene wins),
    to the third a second gene only (which wins).  A single UMI gets the alternation."""
    assert 1 <= U <= n <= 256
    first = [(POOL0[i], [_genes(i)[0]]) for i in range(U)]
    rest = []
    n_recv = max(1, min(U, (2 * (n - U) + 2) // 5))
    for j in range(n - U):
        i, p = j % n_recv, j // n_recv
        kind = 1 if U == 1 else i % 3
        rest.append((POOL0[i], [_genes(i)[(0, (p + 1) % 2, 1)[kind]]]))
    return _finish(first, rest, order, 1000 * U + n)


def build_one_heavy(order="owners-last"):
    """192 reads of one UMI (two genes, a unique winner) and 64 distinct UMIs: owners-last puts the 192 in front, so that the
    other 64 owners are claimed in the last key round"""
    g1, g2 = _genes(0)
    heavy = [(POOL0[0], [g1])] * 120 + [(POOL0[0], [g2])] * 72
    rest = [(POOL0[i], [_genes(i)[0]]) for i in range(1, 65)]
    if order == "owners-last":
        return _finish(rest, heavy, "owners-last", 77)
    return _finish(heavy[:1] + rest, heavy[1:], order, 78)


def build_small(n, U):
    """n <= 64 keys: one key round, the table at its 128-slot floor"""
    assert U <= n <= 64
    return build_boundary(U, n)


MANY = (4, 5, 6, 7, 8)


def build_parked(n_plain, extra_genes=None, order="owners-first"):
    """n_plain single-gene UMIs (every fourth with a repeated read), then five UMIs seen with 4 .. 8 genes - the first gene the
    unique winner of the even ones, all genes tied in the odd ones - whose keys beyond the third gene are parked; with
    owners-first their slots are claimed after n_plain others, i.e. they are owners of a dense round beyond the first when
    n_plain >= 64.  extra_genes: one more UMI with that many genes (9: more than the merge holds, the bucket is diverted)."""
    first = [(POOL0[i], [_genes(i)[0]]) for i in range(n_plain)]
    rest = [(POOL0[i], [_genes(i)[0]]) for i in range(0, n_plain, 4)]
    many = list(MANY) + ([extra_genes] if extra_genes else [])
    for k, ng in enumerate(many):
        umi = POOL0[n_plain + k]
        refs = [(2 * (k + 3 * q)) % N_TXP for q in range(ng)]   # even refs: distinct genes under both maps
        assert len(set(refs)) == ng
        first.append((umi, [refs[0]]))
        rest += [(umi, [r]) for r in refs[1:]]
        if k % 2 == 0:
            rest.append((umi, [refs[0]]))
    return _finish(first, rest, order, 5000 + n_plain + (extra_genes or 0))


def bucket0_stats(reads):
    """(n, U, rank of every UMI by first appearance, {umi: {ref: reads}}) of bucket 0, and the reads of bucket 1 - from numpy alone"""
    umis = np.array([r[0] for r in reads], dtype=np.uint64)
    assert all(len(r[1]) == 1 for r in reads) and int(umis.max()) < 0xFFFFFFFF
    b = bucket_of_lg1(umis)
    per, rank = {}, {}
    for (u, refs), bk in zip(reads, b):
        if bk == 0:
            rank.setdefault(u, len(rank))
            per.setdefault(u, {})
            per[u][refs[0]] = per[u].get(refs[0], 0) + 1
    return int((b == 0).sum()), len(per), rank, per, int((b == 1).sum())


def expected_row_crlike(reads):
    """cr-like without USA and with the identity map: a UMI counts for its most-read gene when that is one gene"""
    per = {}
    for u, refs in reads:
        per.setdefault(u, {})
        per[u][refs[0]] = per[u].get(refs[0], 0) + 1
    row = np.zeros(N_TXP)
    for cnt in per.values():
        m = max(cnt.values())
        w = [g for g, c in cnt.items() if c == m]
        if len(w) == 1:
            row[w[0]] += 1
    return row


def _cfg(resolution, usa):
    num_genes = N_TXP // 2 if usa else N_TXP
    cfg = pkg.WorkerConfig.for_resolution(resolution, usa_mode=usa, num_genes=num_genes, num_rows=(num_genes // 2) * 3 if usa else num_genes,
                                          small_thresh=0)
    t2g = (np.arange(N_TXP, dtype=np.uint32) // 2) if usa else np.arange(N_TXP, dtype=np.uint32)
    return cfg, t2g


def run_case(oracle, reads, resolution, usa):
    """one cell through the library and the oracle, rows bit-exact (the EM resolutions as test_crlike_em of the routes file
    compares them: the oracle fixture in the device's arithmetic); returns the batch's counters"""
    cfg, t2g = _cfg(resolution, usa)
    b, off = rad.encode_cells([(9, reads)], 4, 4)
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off)
        st = q.batch_stats()
        st["n_divert"] = q.resolve_divert_count()
    finally:
        q.close()
    assert_same_result(got, oracle.quant(cfg, t2g, b, off))
    assert st["n_buckets"] == 2 and st["n_overflow_buckets"] == 0, st
    return st


MODES = [("cr-like", False), ("cr-like", True), ("cr-like-em", False), ("cr-like-em", True)]
MODE_IDS = ["crlike", "crlike-usa", "em", "em-usa"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("fill", ["n=U", "n=256"])
@pytest.mark.parametrize("U", BOUNDARY_U)
def test_round_boundaries(oracle, U, fill, mode):
    """U distinct UMIs at every edge of a 64-owner round, each key its own UMI and filled to 256 keys"""
    st = run_case(oracle, build_boundary(U, U if fill == "n=U" else 256), *mode)
    assert st["n_divert"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("order", ["owners-first", "owners-last", "shuffled"])
def test_where_the_owners_are_claimed(oracle, order, mode):
    """the distinct UMIs first and the repeats after, the reverse (192 reads of one UMI, then 64 distinct), shuffled"""
    for reads in (build_boundary(100, 256, order), build_one_heavy(order)):
        st = run_case(oracle, reads, *mode)
        assert st["n_divert"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n,U", [(2, 1), (40, 17), (64, 21), (64, 64)])
def test_one_round_buckets(oracle, n, U, mode):
    """n <= 64: one key round, one rule round, the table's 128-slot floor"""
    st = run_case(oracle, build_small(n, U), *mode)
    assert st["n_divert"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("order", ["owners-first", "shuffled"])
@pytest.mark.parametrize("n_plain", [60, 100, 130])
def test_parked_keys_in_later_rounds(oracle, n_plain, order, mode):
    """UMIs with 4 .. 8 genes among more than 64 UMIs: the merge finds their parked words by slot in whichever round they fall"""
    st = run_case(oracle, build_parked(n_plain, None, order), *mode)
    assert st["n_divert"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_nine_genes_divert_the_bucket(oracle, mode):
    """one UMI with 9 genes, an owner of the second dense round: the bucket is diverted before anything is written, same rows"""
    st = run_case(oracle, build_parked(100, 9), *mode)
    assert st["n_divert"] >= 1, st


def test_builders_fill_bucket_zero(oracle):
    """From numpy alone: every builder puts the intended n and U into bucket 0 and keeps both buckets on the table; the oracle
    gives the rows that follow from the reads (no GPU)."""
    def check(reads, n, U):
        n0, U0, rank, per, n1 = bucket0_stats(reads)
        assert (n0, U0) == (n, U) and 257 <= n0 + n1 <= 512 and 1 <= n1 <= 256, (n0, U0, n1)
        cfg, t2g = _cfg("cr-like", False)
        b, off = rad.encode_cells([(9, reads)], 4, 4)
        want = oracle.quant(cfg, t2g, b, off)
        g, v = want.row(0)
        row = np.zeros(N_TXP)
        row[g] = v
        assert np.array_equal(row, expected_row_crlike(reads))
        return rank, per

    for U in BOUNDARY_U:
        check(build_boundary(U, U), U, U)
        _, per = check(build_boundary(U, 256), 256, U)
        if 1 < U < 256:   # repeated reads, second genes, a unique winner among two genes and a tie
            tops = [sorted(c.values(), reverse=True) for c in per.values()]
            assert any(len(t) == 1 and t[0] > 1 for t in tops)
            assert any(len(t) == 2 and t[0] > t[1] for t in tops) and any(len(t) == 2 and t[0] == t[1] for t in tops)
    for order in ("owners-first", "owners-last", "shuffled"):
        rank, _ = check(build_boundary(100, 256, order), 256, 100)
        rank, per = check(build_one_heavy(order), 256, 65)
        if order == "owners-last":
            assert rank[POOL0[0]] == 0 and len(per[POOL0[0]]) == 2
    for n, U in [(2, 1), (40, 17), (64, 21), (64, 64)]:
        check(build_small(n, U), n, U)
    for n_plain in (60, 100, 130):
        for order in ("owners-first", "shuffled"):
            n_keys = n_plain + (n_plain + 3) // 4 + sum(MANY) + 3
            rank, per = check(build_parked(n_plain, None, order), n_keys, n_plain + 5)
            many = [u for u, c in per.items() if len(c) > 3]
            assert sorted(len(per[u]) for u in many) == list(MANY)
            assert sum(len(per[u]) - 3 for u in many) <= 64   # the parked list holds them
            if order == "owners-first" and n_plain >= 64:
                assert all(rank[u] >= 64 for u in many)
    rank, per = check(build_parked(100, 9), 100 + 25 + sum(MANY) + 3 + 9, 106)
    assert max(len(c) for c in per.values()) == 9 and all(rank[u] >= 64 for u, c in per.items() if len(c) > 3)
