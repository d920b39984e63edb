"""GPU tests of the convert kernels: Quantifier.convert_bam_rad against tests/convert_judge.py's `stated` on the cases of
tests/bam_cases.py, with host bytes and with bytes already on the device.  Everything is exact: the output bytes, the chunk table,
the per-chunk record counts and every stat.  Each call is made twice and the two outputs must be equal.  Shapes derive from
convert_limits()."""
import numpy as np
import pytest

import bam_cases as B
import convert_judge as J
from util import pkg

pytestmark = pytest.mark.gpu
CODES = {"BAD_INPUT": pkg._abi.AFQ_ERR_BAD_INPUT, "UNSUPPORTED": pkg._abi.AFQ_ERR_UNSUPPORTED, "INVALID_ARG": pkg._abi.AFQ_ERR_INVALID_ARG}


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def lim():
    return pkg.convert_limits()


def call(q, c, fb, on_device=False):
    stream, _ = B.stream_of(c)
    bw, uw = J.widths(c["records"])
    kw = dict(n_ref=len(c["ref_names"]), bc_bytes=bw, umi_bytes=uw, filter_best=fb)
    if not on_device:
        return q.convert_bam_rad(stream, B.span_table(c), **kw)
    import torch

    t = torch.from_numpy(np.frombuffer(b"\xFF" * 3 + stream + b"\xFF" * 9, np.uint8).copy()).cuda()   # off a dword boundary, other bytes around it
    return q.convert_bam_rad(None, B.span_table(c), d_ptr=t.data_ptr() + 3, n_bytes=len(stream), **kw)


def same(got, want, what=""):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["nrec"].tolist() == want["nrec"], (what, "nrec")
    assert got["chunk_off"].tolist() == want["chunk_off"], (what, "chunk_off")
    gb = got["bytes"].tobytes()
    if gb != want["bytes"]:
        at = next(i for i, (x, y) in enumerate(zip(gb, want["bytes"])) if x != y)
        raise AssertionError((what, "bytes differ first at", at, gb[max(0, at - 8):at + 24].hex(), want["bytes"][max(0, at - 8):at + 24].hex()))


def check(q, lim, c):
    out = {}
    for fb in c["filters"]:
        want = J.stated(c["records"], fb, n_ref=len(c["ref_names"]), lane_alns=lim["lane_alns"])
        for on_device in (False, True):
            a, b = call(q, c, fb, on_device), call(q, c, fb, on_device)
            same(a, want, f"{c['name']} filter_best={fb} device={on_device}")
            same(b, want, f"{c['name']} filter_best={fb} device={on_device} (second call)")
        out[fb] = want
    return out


def test_every_case_equals_the_stated_semantics(q, lim):
    seen, cases = set(), B.device_cases(lim)   # (the container cases are one stream: tests/test_gpu_convert_cli.py reads their files)
    for c in cases:
        for fb, w in check(q, lim, c).items():
            seen.add(c["name"])
            if c["name"] == "all_dropped":
                assert w["stats"]["n_chunks"] == 0 and w["bytes"] == b"" and w["chunk_off"] == [0]
            if c["name"] == "run_lengths":
                assert w["stats"]["n_long_runs"] == 4   # 63, 64, 65 and lane_alns + 1
            if c["name"] == "long_run_across_tiles" and fb:
                assert w["stats"]["n_alignments_written"] == 5 and w["stats"]["n_alignments_in"] == 3002
            if c["name"] == "dropped_span_between":
                assert w["stats"]["n_runs"] == 2 and w["stats"]["n_dropped_by_flag"] == 5
            if c["name"] == "two_n":
                assert w["stats"]["n_runs_dropped_n"] == 3 and w["stats"]["n_runs_written"] == 5
    assert len(seen) == len(cases) >= 26


@pytest.mark.parametrize("i", range(6))
def test_chunk_boundaries(q, lim, i):
    c = B.chunk_cases()[i]
    w = check(q, lim, c)[False]
    want_chunks = {"runs_10000": [10000], "runs_10001": [10001], "runs_10002": [10001, 1], "runs_20002": [10001, 10001], "runs_20003": [10001, 10001, 1],
                   "dropped_run_on_the_boundary": [10001, 1]}[c["name"]]
    assert w["nrec"] == want_chunks
    assert w["stats"]["n_runs_written"] > lim["scan_block"]   # more than one workgroup of the flag scans, and of the layout scan


@pytest.mark.parametrize("i", range(len(B.error_cases())))
def test_errors_name_the_record_and_leave_the_context_usable(q, lim, i):
    c, fb, code, index = B.error_cases()[i]
    if c["name"] not in B.MALFORMED:   # the judge refuses the same record (a malformed record has no dict to judge: its bytes are the case)
        with pytest.raises(J.Refusal) as je:
            J.stated(c["records"], fb, n_ref=len(c["ref_names"]))
        assert je.value.index == index
    for on_device in (False, True):
        with pytest.raises(pkg.AfqError) as e:
            call(q, c, fb, on_device)
        assert e.value.code == CODES[code] and f"record {index}:" in str(e.value), str(e.value)
    check(q, lim, B.name_cases()[0])   # the context serves again afterwards


def test_the_score_errors_are_raised_only_where_a_run_is_written(q, lim):
    c = B.error_cases()[8][0]
    assert c["name"] == "no_score"
    same(call(q, c, False), J.stated(c["records"], False, n_ref=len(c["ref_names"]), lane_alns=lim["lane_alns"]), "no AS, no filter")


def test_bad_arguments(q):
    c = B.name_cases()[0]
    stream, offs = B.stream_of(c)
    for spans in ([1], [0, offs[3], offs[2]], [0, len(stream)]):
        with pytest.raises(pkg.AfqError) as e:
            q.convert_bam_rad(stream, spans, n_ref=7, bc_bytes=4, umi_bytes=4)
        assert e.value.code == CODES["INVALID_ARG"] and "span" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.convert_bam_rad(stream, [0], n_ref=7, bc_bytes=3, umi_bytes=4)
    assert e.value.code == CODES["INVALID_ARG"]
    got = q.convert_bam_rad(b"", [], n_ref=7, bc_bytes=4, umi_bytes=4)
    assert len(got["bytes"]) == 0 and got["chunk_off"].tolist() == [0] and got["stats"]["n_records"] == 0
