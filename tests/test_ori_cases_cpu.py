"""tests/ori_cases.py on the CPU: the rewrite changes bit 31 of the alignment words and nothing else, on every layout that
tests/test_gpu_orientation.py uses; the witnesses reach the floors that the GPU tests rely on (stated here, checked here, not
tuned to what a device gives); and the oracle, which strips the bit once at load, gives the twin's result on every pattern for
all seven resolutions - it has to pass this alone before the device stands against anything."""
import numpy as np
import pytest

import ori_cases as oc
from util import assert_same_result, pkg

rad = pkg.rad
RESOLUTIONS = ("trivial", "cr-like", "cr-like-em", "parsimony", "parsimony-em", "parsimony-gene", "parsimony-gene-em")
# the label-length classes each input is used for (tests/test_gpu_orientation.py, "label lengths")
CLASSES_NAMED = {"tailed": ("1", "2", "3-4", "5-8", "9-16", "17-64"), "tailed-usa": ("1", "2", "3-4", "5-8", "9-16", "17-64"),
                 "wide-labels": (">64",), "wide-labels-usa": (">64",)}


@pytest.mark.parametrize("pattern", oc.PATTERNS)
@pytest.mark.parametrize("name", oc.NAMES)
def test_the_rewrite_changes_bit_31_of_the_alignment_words_and_nothing_else(name, pattern):
    inp = oc.inputs(name)
    twin, new = inp.twin, inp.rewritten(pattern, seed=3)
    assert len(new.data) == len(twin.data) and np.array_equal(new.off, twin.off) and new.data is not twin.data
    # every byte but the top byte of an alignment word is the twin's, and of those the low seven bits are
    recs, w_twin, rec_of, j = twin.words()
    at = recs.first[rec_of] + (4 + twin.pos_bytes) * j
    diff = np.flatnonzero(new.data != twin.data)
    assert np.isin(diff, at + 3).all()
    assert not ((new.data[at + 3] ^ twin.data[at + 3]) & 0x7F).any()
    assert (w_twin >> 31).all(), "the twin is what every builder makes today: all set"
    # rad.decode_chunk, which masks, reads the twin's cells out of the rewritten bytes
    for o in twin.off[:: max(1, len(twin.off) // 40)]:
        a = rad.decode_chunk(bytes(new.data), int(o), twin.bc_bytes, twin.umi_bytes, twin.pos_bytes, with_pos=True)
        assert a == rad.decode_chunk(bytes(twin.data), int(o), twin.bc_bytes, twin.umi_bytes, twin.pos_bytes, with_pos=True)
    assert new.cells() == inp.reads
    # the bits are as the rule says, stated here a second time and word by word
    _, w, _, _ = new.words()
    bits = (w >> 31).tolist()
    na, r, jj = recs.na[rec_of].tolist(), recs.rec[rec_of].tolist(), j.tolist()
    rule = {"clear": lambda k: 0, "alternate": lambda k: jj[k] % 2, "first-clear": lambda k: int(jj[k] != 0),
            "last-clear": lambda k: int(jj[k] != na[k] - 1), "per-read": lambda k: r[k] % 2}.get(pattern)
    if rule is not None:
        assert bits == [rule(k) for k in range(len(bits))]
    else:
        assert 0 < sum(bits) < len(bits)
        assert len(bits) < 500 or 0.4 * len(bits) < sum(bits) < 0.6 * len(bits)      # (a fair coin: 5 sigma at 500 words is 0.39 ... 0.61)
        assert bits == (inp.twin.reoriented("random", seed=3).words()[1] >> 31).tolist(), "a seeded coin"
        assert bits != (inp.rewritten("random", seed=4).words()[1] >> 31).tolist()
    if pattern in ("first-clear", "last-clear"):
        clear_per_record = np.bincount(rec_of, weights=1 - np.asarray(bits), minlength=len(recs.na))
        assert (clear_per_record[recs.na > 0] == 1).all()
    # refs ascending and distinct in every record, as they were
    assert all(all(a < b for a, b in zip(refs, refs[1:])) for reads in inp.reads for _, refs in reads)


@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("name", oc.FUZZ)
def test_fuzz_batches_hold_mixed_pairs_that_share_a_umi_and_that_lie_one_base_apart(name, pattern):
    """Reads of one label that meet with different raw words: under one UMI (one vertex, one key to cr-like) and under UMIs one
    base apart (an edge whose label test compares two labels).  At least 100 pairs of each kind a batch."""
    pairs = oc.mixed_label_pairs(oc.inputs(name).rewritten(pattern))
    print(f"\n{name} {pattern}: {pairs}")
    assert sum(t["same_umi"] for t in pairs.values()) >= oc.FUZZ_FLOOR
    assert sum(t["one_base"] for t in pairs.values()) >= oc.FUZZ_FLOOR


@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("name", list(CLASSES_NAMED))
def test_every_label_length_class_that_a_case_names_is_reached(name, pattern):
    pairs = oc.mixed_label_pairs(oc.inputs(name).rewritten(pattern))
    print(f"\n{name} {pattern}: {pairs}")
    assert set(CLASSES_NAMED[name]) <= oc.classes_reached(pairs)


@pytest.mark.parametrize("name", [n for n in oc.NAMES if n != "structured-3"])
def test_two_ref_keys_see_every_combination_of_bits_and_raw_words_out_of_order(name):
    """Under `random`: two-ref records with the bit clear on both words, on the first only and on the second only (t1's bit 31
    next to t0's field in `t0 << 31 | t1`), and records whose raw words are not ascending."""
    case = oc.inputs(name).rewritten("random")
    assert all(n > 0 for n in oc.two_ref_bleed(case).values())
    assert oc.unsorted_raw(case) > 0
    assert oc.unsorted_raw(oc.inputs(name).twin) == 0 and not any(oc.two_ref_bleed(oc.inputs(name).twin).values())


def test_the_witnesses_count_what_they_say():
    """By hand: cell 0 holds label (1, 2) three times with two raw spellings under UMI 5 and a third one base away; cell 1 the
    same label once (no pair across cells)."""
    S = oc.BIT
    cells = [(7, [(5, [1, 2]), (5, [1, 2]), (5, [1, 2]), (4, [1, 2]), (5, [3])]), (8, [(5, [1, 2])])]
    b, off = rad.encode_cells(cells, 4, 4, fw_bit=False)
    w = np.frombuffer(b, np.uint32).copy()
    recs = oc.walk(b, off, 4, 4)
    first = (recs.first // 4).tolist()
    w[first[0]] |= S                       # (1, 0)
    w[first[1]] |= S                       # (1, 0)
    w[first[2] + 1] |= S                   # (0, 1): raw words 1, S | 2 - ascending
    case = oc.Case(w.view(np.uint8), off)  # record 3: (0, 0)
    p = oc.mixed_label_pairs(case)
    assert p["2"] == {"pairs": 5, "same_umi": 2, "one_base": 3} and all(not any(p[k].values()) for k in oc.LENGTH_CLASSES if k != "2")
    assert oc.two_ref_bleed(case) == {(0, 0): 2, (0, 1): 1, (1, 0): 2}
    assert oc.unsorted_raw(case) == 2
    assert case.cells() == [r for _, r in cells]


# ------------------------------------------------------------------------------------------------------- the oracle is invariant

def _oracle(oracle, inp, case, res, dump_eq):
    kw = dict(dump_eq=True, num_bootstraps=3, boot_seed=41) if res.endswith("-em") else dict(dump_eq=dump_eq)
    cfg = inp.cfg(res, **kw)
    return cfg, oracle.quant(cfg, np.asarray(inp.t2g, np.uint32), case.data, case.off, n_threads=8)


def _same(a, b, cfg, what):
    assert_same_result(a, b, what=what)
    if cfg.dump_eq:
        for f in ("cell_ptr", "label_ptr", "labels", "count"):
            assert np.array_equal(getattr(a.eqclasses, f), getattr(b.eqclasses, f)), (what, f)
    if cfg.num_bootstraps:
        for f in ("mean_ptr", "mean_col", "var_ptr", "var_col"):
            assert np.array_equal(getattr(a.bootstraps, f), getattr(b.bootstraps, f)), (what, f)
        for f in ("mean_val", "var_val"):
            assert np.array_equal(getattr(a.bootstraps, f).view(np.uint32), getattr(b.bootstraps, f).view(np.uint32)), (what, f)


@pytest.mark.parametrize("res", RESOLUTIONS)
@pytest.mark.parametrize("name", ["base", "usa", "structured", "wide-labels-usa", "tailed"])
def test_the_oracle_gives_the_twins_result_on_every_pattern(oracle, name, res):
    """All seven resolutions, USA and not, with -d classes and, for the -em resolutions, three bootstraps under a fixed seed."""
    inp = oc.inputs(name)
    dump = res in ("cr-like", "parsimony", "parsimony-gene")
    cfg, want = _oracle(oracle, inp, inp.twin, res, dump)
    assert want.val.sum() > 0
    for pattern in oc.PATTERNS:
        _, got = _oracle(oracle, inp, inp.rewritten(pattern), res, dump)
        _same(got, want, cfg, f"{name} {res} {pattern}")
