"""How the GPU tests that run a case through SEVERAL record passes (tests/test_gpu_far_offsets.py, tests/test_gpu_rad_pass_sweep.py)
call each pass and compare its result with the family's judge: `run(family, q, case, ori, data, off, **dev)` with host bytes `data`,
or data = None and d_ptr / n_bytes for bytes on the device; `same(family, got, want, case, what)` as the family's own GPU tests
compare.  Nothing here decides what is right."""
import contextlib

import atac_dedup_cases as AD
import atac_gpl_cases as AG
import atac_sort_cases as AS
import collate_multi_cases as CM
import gpl_cases as G
import gpl_multi_cases as MC


def same_collated(got, want, what, cell=False):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["nrec"].tolist() == want["nrec"], (what, "nrec")
    assert not cell or got["cell"].tolist() == want["cell"], (what, "cell")
    assert got["chunk_off"].tolist() == want["chunk_off"], (what, "chunk_off")
    gb = got["bytes"].tobytes()
    if gb != want["bytes"]:
        at = next((i for i, (x, y) in enumerate(zip(gb, want["bytes"])) if x != y), min(len(gb), len(want["bytes"])))
        raise AssertionError((what, "bytes differ first at", at, gb[max(0, at - 8):at + 24].hex(), want["bytes"][max(0, at - 8):at + 24].hex()))


@contextlib.contextmanager
def pos_bytes(q, c):
    q.set_aln_extra_bytes(c.get("pos_bytes", 0))
    try:
        yield
    finally:
        q.set_aln_extra_bytes(0)


def run_gpl(q, c, ori, data, off, **dev):
    with pos_bytes(q, c):
        return q.gpl_hist_rad(data, off, bc_bytes=c["bc_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori, **dev)


def run_gpl_multi(q, c, ori, data, off, **dev):
    with pos_bytes(q, c):
        return q.gpl_multi_hist_rad(data, off, c["entries"], b0_bytes=c["b0_bytes"], b1_bytes=c["b1_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori, **dev)


def run_atac_gpl(q, c, ori, data, off, **dev):
    return q.atac_gpl_hist_rad(data, off, c["blens"], bc_bytes=c["bc_bytes"], **dev)


def run_atac_sort(q, c, ori, data, off, **dev):
    return q.atac_sort_rad(data, off, c["obs"], c["cor"], c["ref_lengths"], bc_bytes=c["bc_bytes"], **dev)


def run_collate(q, c, ori, data, off, **dev):
    obs = sorted(c["corrections"])
    with pos_bytes(q, c):
        return q.collate_rad(data, off, obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=c["bc_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori, **dev)


def run_collate_multi(q, c, ori, data, off, **dev):
    with pos_bytes(q, c):
        return q.collate_multi_rad(data, off, *CM.args(c), b0_bytes=c["b0_bytes"], b1_bytes=c["b1_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori, **dev)


def run_atac_collate(q, c, ori, data, off, **dev):
    obs = sorted(c["corrections"])
    return q.atac_collate_rad(data, off, obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=c["bc_bytes"], **dev)


def run_atac_dedup(q, c, ori, data, off, **dev):
    return q.atac_dedup_rad(data, off, bc_bytes=c["bc_bytes"], **dev)


# family -> (the entry point, how the family's own tests compare a result with its judge's)
PASSES = {
    "gpl": (run_gpl, lambda got, want, c, what: G.same_hist(got, want, what)),
    "gpl multi": (run_gpl_multi, lambda got, want, c, what: MC.same_pairs(got, want, what)),
    "atac gpl": (run_atac_gpl, lambda got, want, c, what: AG.same(got, want, what)),
    "atac sort": (run_atac_sort, lambda got, want, c, what: AS.same(got, want, what)),
    "collate": (run_collate, lambda got, want, c, what: same_collated(got, want, what)),
    "collate multi": (run_collate_multi, lambda got, want, c, what: same_collated(got, want, what)),
    "atac collate": (run_atac_collate, lambda got, want, c, what: same_collated(got, want, what, cell=True)),
    "atac dedup": (run_atac_dedup, lambda got, want, c, what: AD.same_as_judge(got, c, what)),   # (it judges the case itself)
}


def run(family, q, case, ori, data, off, **dev):
    return PASSES[family][0](q, case, ori, data, off, **dev)


def same(family, got, want, case, what=""):
    PASSES[family][1](got, want, case, what)
