"""The device before the judge of tests/atac_dedup_judge.py on every case of tests/atac_dedup_cases.py: afq_atac_dedup_rad by the
plain route and by the eight-range pipeline (with its run list, with a list that overflows after 400 runs, without one), from host
bytes and from bytes on the device; the column-level afq_atac_dedup; one context across a wrap batch and an ordinary one; and the
`afquant atac deduplicate` command.  The comparisons with the oracle stay where they are (tests/test_gpu_atac.py); what the cases
reach is shown without a device by tests/test_atac_dedup_judge_cpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import atac_dedup_cases as A
import atac_dedup_judge as J
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")

PIPE, CAP = "AFQ_TEST_ATAC_PIPE_BYTES", "AFQ_TEST_ATAC_RUN_CAP"
ROUTES = {"plain": {}, "piped": {PIPE: "1"}, "piped-list-overflows-after-400": {PIPE: "1", CAP: "400"}, "piped-no-run-list": {PIPE: "1", CAP: "0"}}
# (the sixteen parse cases go four to a context: one barcode width, the four byte alignments)
GROUPS = {n: [n] for n in A.all_case_names() if not n.startswith("parse")}
GROUPS.update({"parse_%d" % w: ["parse_%d_%d" % (w, p) for p in range(4)] for w in A.WIDTHS})


def _q(profile=True):
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=profile)
    return pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)


def _route(monkeypatch, route):
    for k in (PIPE, CAP):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def _dedup(q, case, on_device):
    if not on_device:
        return q.atac_dedup_rad(case["data"], case["off"], bc_bytes=case["bc_bytes"])
    import torch

    t = torch.from_numpy(case["data"]).cuda()
    return q.atac_dedup_rad(None, case["off"], bc_bytes=case["bc_bytes"], d_ptr=t.data_ptr(), n_bytes=len(case["data"]))


def _launches(case, route):
    """(parse, dedup) launches: a batch with a reference id of 65536 and more is done again in one piece by the 16-byte-record
    kernel, whichever route it came by; else one launch of each, or one per range"""
    return (1, 2) if case["wide"] else (1, 1) if route == "plain" else (8, 8)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("group", list(GROUPS))
def test_device_from_bytes_before_the_judge(monkeypatch, group, route):
    """Rows, counts, barcodes and the five tallies are the judge's; the cells that were walked are the ones built to fail the
    proof; the launch counts show the route."""
    _route(monkeypatch, route)
    q = _q()
    try:
        for name in GROUPS[group]:
            case = A.get_case(name)
            for on_device in (False, True):
                what = "%s, %s, %s bytes:" % (name, route, "device" if on_device else "host")
                got = _dedup(q, case, on_device)
                kt = q.kernel_times()
                A.same_as_judge(got, case, what)
                assert got[6]["n_fallback_cells"] == case["n_fallback"], (what, got[6])
                assert (kt["k_atac_parse"][1], kt["k_atac_dedup"][1]) == _launches(case, route), (what, kt)
    finally:
        q.close()


@pytest.mark.parametrize("group", list(GROUPS))
def test_device_from_columns_before_the_judge(group):
    """afq_atac_dedup on the kept fragments of every case: rows and counts (it has no tallies)."""
    q = _q()
    try:
        for name in GROUPS[group]:
            case = A.get_case(name)
            got = q.atac_dedup(*A.kept_columns(case))
            kt = q.kernel_times()
            A.same_as_judge(got, case, name + ", columns:", rows_only=True)
            assert kt["k_atac_dedup"][1] == (2 if case["wide"] else 1), (name, kt)
    finally:
        q.close()


@pytest.mark.parametrize("route", ["plain", "piped"])
@pytest.mark.parametrize("order", [("wrap", "filter", "wrap"), ("filter", "wrap", "packing_wide_last", "wrap", "filter")])
def test_one_context_across_wrap_batches_and_ordinary_ones(monkeypatch, order, route):
    """The tally of the wrapped runs starts at zero for every batch - after a wrap batch, and after a batch that was done
    again because of a wide reference id."""
    _route(monkeypatch, route)
    q = _q(profile=False)
    try:
        for k, name in enumerate(order):
            case = A.get_case(name)
            A.same_as_judge(_dedup(q, case, on_device=bool(k % 2)), case, "%s as batch %d of %s, %s:" % (name, k, order, route))
    finally:
        q.close()


@pytest.mark.parametrize("rev", [False, True])
def test_afquant_atac_deduplicate_writes_the_judges_bed_and_log(tmp_path, rev):
    """The wrap cell and a cell on the 2000-base boundary in a directory: map.bed is the judge's multiset of lines - a 0 in the
    count column among them - and the four counters on stderr are the judge's, "deduplicated 5" among them."""
    case = A.cli_case()
    want = A.judged(case)
    names = ["chr1", "chr2", "chr3", "chrX"]
    d = tmp_path / "in"
    os.makedirs(d)
    (d / "generate_permit_list.json").write_text(json.dumps({"velo_mode": False}))
    (d / "collate.json").write_text(json.dumps({"compressed_output": False}))
    (d / "map.collated.rad").write_bytes(rad.rad_prelude_atac(names, [1 << 20] * 4, len(case["off"])) + case["data"].tobytes())
    r = subprocess.run([CLI, "atac", "deduplicate", "-i", str(d), "-t", "3"] + ([] if rev else ["-d", "fw"]), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exp = []
    for i, (bc, _) in enumerate(case["cells"]):
        exp += J.bed_lines(want.rows[want.cell_ptr[i]:want.cell_ptr[i + 1]], bc, names, 16, rev)
    got = (d / "map.bed").read_text().splitlines()
    assert sorted(got) == sorted(exp) and len(got) == len(want.rows) - want.n_long_fragments == 12
    assert sorted(ln.split("\t")[4] for ln in got if ln.startswith("chrX\t") and int(ln.split("\t")[1]) % 1000) == ["0", "0", "1", "1", "65535"]
    for line in J.log_lines(want):
        assert line + "\n" in r.stderr, (line, r.stderr)
    assert "Number of records that are deduplicated 5\n" in r.stderr
