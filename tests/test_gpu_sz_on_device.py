"""GPU tests of --sz-on-device: `afquant quant` and `afquant atac deduplicate` on a map.collated.rad.sz that is decoded on the device
and stays there (afq_snappy_frame_decode_device, afq_collated_chunk_table, afq_submit_device) write, byte for byte, what they write
with the file decoded on the host; and the door's refusals."""
import gzip
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import multi_bc_cases as mb
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
synth = pkg.synth
sn = importlib.import_module("alevin-fry_amd.synth_native")
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")


def to_sz(d, chunk=60000):
    """map.collated.rad of directory d becomes map.collated.rad.sz, frame chunks cut every `chunk` bytes; returns the stream"""
    body = (d / "map.collated.rad").read_bytes()
    (d / "map.collated.rad").unlink()
    stream = rad.snappy_frame_encode(body, chunk=chunk)
    (d / "map.collated.rad.sz").write_bytes(stream)
    meta = json.loads((d / "collate.json").read_text())
    meta["compressed_output"] = True
    (d / "collate.json").write_text(json.dumps(meta))
    return stream, body


def quant_dir(d, s, pad=0, pos_bytes=0, long_names=0, chunk=7000):
    """a compressed input directory of synth `s`; `pad` lengthens one reference name (the prelude's length decides the shift),
    long_names makes every name that many characters longer (a prelude of more than one frame chunk); frame chunks of `chunk` bytes,
    so that these small files are streams of a dozen chunks and more"""
    b, off = rad.encode_cells_np(s.cell_nrec, s.cell_bc, s.umi, s.na, s.refs, pos_bytes=pos_bytes)
    names = [f"T{t}" + "n" * long_names for t in range(len(s.tid_to_gid))]
    names[0] += "p" * pad
    rows = [(names[t], f"G{gid >> 1}", "S" if gid % 2 == 0 else "U") if s.usa else (names[t], f"G{gid}") for t, gid in enumerate(s.tid_to_gid.tolist())]
    tg = rad.write_quant_input_dir(str(d), np.asarray(b).tobytes(), len(off), names, rows, cblen=16, ulen=s.umi_len, pos_bytes=pos_bytes)
    stream, body = to_sz(d, chunk)
    first_chunk = len(body) - len(np.asarray(b).tobytes())
    return tg, stream, first_chunk


def strip(meta, dirs):
    if isinstance(meta, dict):
        return {k: strip(v, dirs) for k, v in meta.items() if k not in ("cmd", "cmdline")}
    if isinstance(meta, list):
        return [strip(v, dirs) for v in meta]
    if isinstance(meta, str):
        for x in dirs:
            meta = meta.replace(x, "<out>")
    return meta


def tree(out):
    """every file under `out` -> its bytes (gzip members unpacked: their headers carry a time; quant.json parsed, `cmd` apart)"""
    got = {}
    for root, _, files in os.walk(out):
        for f in files:
            p = os.path.join(root, f)
            rel = os.path.relpath(p, out)
            if f.endswith(".gz"):
                got[rel] = gzip.open(p).read()
            elif f == "quant.json":
                got[rel] = strip(json.load(open(p)), [str(out)])
            else:
                got[rel] = open(p, "rb").read()
    return got


def both_doors(tmp_path, d, tg, res, extra=(), env=None):
    outs = []
    for door in ("closed", "open"):
        out = tmp_path / f"out_{door}"
        r = subprocess.run([CLI, "quant", "-i", str(d), "-m", tg, "-o", str(out), "-r", res, "-t", "2", *extra] + (["--sz-on-device"] if door == "open" else []),
                           capture_output=True, text=True, env={**os.environ, **(env or {})})
        assert r.returncode == 0, (door, r.stderr)
        outs.append((tree(out), r.stderr))
    (closed, _), (opened, err_open) = outs
    assert set(closed) == set(opened) and "alevin/quants_mat.mtx" in closed and len(closed["alevin/quants_mat.mtx"].splitlines()) > 10
    for f in closed:
        assert closed[f] == opened[f], f
    return closed, err_open


SYNTH = dict(num_genes=120, txp_per_gene=2, dup=0.5, cross=0.3, umi_err=0.02)
CELLS = [2500, 700, 260, 120, 60, 7]


# (what, resolution, USA mode, extra arguments, pos_bytes): between them the preludes have every length modulo 4, so that the
# decoded chunks land at every shift = (4 - first_chunk % 4) % 4 - SHIFTS[k] is case k's, asserted in the run that compares
SHIFTS = [1, 0, 3, 2, 3, 0]
QUANT_CASES = [("cr-like", "cr-like", False, [], 0), ("parsimony-em usa", "parsimony-em", True, [], 0), ("subset", "cr-like", False, ["--quant-subset"], 0),
               ("dump", "cr-like", True, ["-d"], 0), ("positions", "cr-like", False, [], 2), ("dump em", "parsimony-em", False, ["-d"], 0)]


@pytest.mark.parametrize("k", range(len(QUANT_CASES)), ids=[c[0] for c in QUANT_CASES])
def test_quant_writes_the_same_files_with_the_door_open(tmp_path, k):
    what, res, usa, extra, pos_bytes = QUANT_CASES[k]
    s = synth.synth(88 + k, CELLS, usa=usa, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s, pad=k % 4, pos_bytes=pos_bytes)
    assert (4 - first_chunk % 4) % 4 == SHIFTS[k] and set(SHIFTS) == {0, 1, 2, 3}, (first_chunk, "this compared run's shift; the cases meet all four")
    extra = list(extra)
    if "--quant-subset" in extra:
        sub = tmp_path / "subset.txt"
        sub.write_text("\n".join(rad.int_to_seq(int(s.cell_bc[i]), 16) for i in (0, 2, 3, 5)) + "\n")
        extra.append(str(sub))
    closed, _ = both_doors(tmp_path, d, tg, res, extra)
    if "--quant-subset" in extra:
        assert len(closed["alevin/quants_mat_rows.txt"].split()) == 4
    if "-d" in extra:
        assert len(closed["alevin/gene_eqclass.txt.gz"]) > 10 and "alevin/geqc_counts.mtx" in closed


def test_quant_with_a_prelude_longer_than_a_frame_chunk(tmp_path):
    s = synth.synth(70, CELLS, usa=False, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s, long_names=600, chunk=60000)
    assert first_chunk > 2 * 60000, "the prelude fills more than two frame chunks"
    both_doors(tmp_path, d, tg, "cr-like")


def test_quant_in_several_batches_whose_spans_start_inside_frame_chunks(tmp_path):
    s = synth.synth(71, [1500, 1400, 1300, 1200, 700, 260, 120, 60, 7], usa=True, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s, pad=1)
    closed, err = both_doors(tmp_path, d, tg, "cr-like", ["-d"], env={"AFQ_TEST_QUEUE_BATCH_BYTES": "40000", "AFQ_HOST_TIMING": "1"})
    assert sum("batches" in ln and "device 0" in ln for ln in err.splitlines()) == 1
    n_batches = int(next(ln for ln in err.splitlines() if "device 0:" in ln).split("device 0:")[1].split("batches")[0])
    assert n_batches >= 4, err
    for lap in ("sz: prelude chunks", "sz: upload + decode", "sz: chunk table"):
        assert lap in err, lap
    assert "map + snappy decode" not in err


@pytest.mark.parametrize("layout", [(2, 4, 4), (4, 4, 4)], ids=["b0 u16", "b0 u32"])
def test_multi_barcode_quant(tmp_path, layout):
    case = mb.cli_case(layout)
    d = tmp_path / "in"
    tg = mb.write_cli_dir(d, case)
    to_sz(d, chunk=1000)
    closed, _ = both_doors(tmp_path, d, tg, "cr-like")
    sub = tmp_path / "subset.txt"
    sub.write_text("\n".join(rad.int_to_seq(b, 4 * case.w1) for b in (mb.CLI_CELL_BARCODES[1] & mb.ones(case.w1), mb.CLI_CELL_BARCODES[3] & mb.ones(case.w1))) + "\n")
    subset, _ = both_doors(tmp_path, d, tg, "cr-like", ["--quant-subset", str(sub)])
    assert 0 < len(subset["alevin/quants_mat_rows.txt"].split()) < len(closed["alevin/quants_mat_rows.txt"].split())


def atac_dir(d, compressed=True):
    data, off = sn.generate_atac(seed=12, n_cells=40, frags_per_cell=500, n_refs=3, ref_len=100000, flen_sigma=1.5)
    pre = rad.rad_prelude_atac(["chr1", "chr2", "chrX"], [100000] * 3, len(off))
    os.makedirs(d)
    (d / "generate_permit_list.json").write_text(json.dumps({"velo_mode": False}))
    (d / "collate.json").write_text(json.dumps({"compressed_output": False}))
    (d / "map.collated.rad").write_bytes(pre + data.tobytes())
    return to_sz(d)[0] if compressed else None


def test_atac_deduplicate_writes_the_same_bed_and_counters(tmp_path):
    runs = []
    for door in ("closed", "open"):
        d = tmp_path / door
        atac_dir(d)
        r = subprocess.run([CLI, "atac", "deduplicate", "-i", str(d), "-t", "3"] + (["--sz-on-device"] if door == "open" else []), capture_output=True, text=True)
        assert r.returncode == 0, (door, r.stderr)
        runs.append(((d / "map.bed").read_bytes(), [ln for ln in r.stderr.splitlines() if ln.startswith(("finished parsing", "Number of records"))]))
    assert runs[0] == runs[1] and len(runs[0][0].splitlines()) > 1000 and len(runs[0][1]) == 5


def test_the_door_is_ignored_on_an_uncompressed_directory(tmp_path):
    d = tmp_path / "in"
    atac_dir(d, compressed=False)
    r = subprocess.run([CLI, "atac", "deduplicate", "-i", str(d), "--sz-on-device"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr.count("--sz-on-device: map.collated.rad is not compressed; the option is ignored") == 1, r.stderr
    s = synth.synth(72, [300, 60, 7], usa=False, **SYNTH)
    b, off = s.encode()
    names = [f"T{t}" for t in range(len(s.tid_to_gid))]
    tg = rad.write_quant_input_dir(str(tmp_path / "q"), np.asarray(b).tobytes(), len(off), names, [(names[t], f"G{g}") for t, g in enumerate(s.tid_to_gid.tolist())], cblen=16, ulen=s.umi_len)
    r = subprocess.run([CLI, "quant", "-i", str(tmp_path / "q"), "-m", tg, "-o", str(tmp_path / "qo"), "-r", "cr-like", "--sz-on-device"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr.count("the option is ignored") == 1 and (tmp_path / "qo" / "alevin" / "quants_mat.mtx").exists(), r.stderr


def test_refusals(tmp_path):
    s = synth.synth(73, CELLS, usa=False, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s)
    out = tmp_path / "out"
    base = [CLI, "quant", "-i", str(d), "-m", tg, "-o", str(out), "-r", "cr-like", "--sz-on-device"]
    r = subprocess.run(base + ["--devices", "0,0"], capture_output=True, text=True)
    assert r.returncode != 0 and "--sz-on-device takes one device" in r.stderr and not out.exists(), r.stderr
    # one bit of the last data chunk's CRC
    at, starts = 0, []
    while at < len(stream):
        starts.append(at)
        at += 4 + int.from_bytes(stream[at + 1:at + 4], "little")
    assert len(starts) >= 9, "the identifier and eight data chunks at the least"
    bad = bytearray(stream)
    bad[starts[-1] + 5] ^= 0x10
    (d / "map.collated.rad.sz").write_bytes(bytes(bad))
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode != 0 and f"map.collated.rad.sz: snappy CRC mismatch (chunk {len(starts) - 2})" in r.stderr and not out.exists(), r.stderr
    # the file as it was: the command serves again
    (d / "map.collated.rad.sz").write_bytes(stream)
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0 and out.exists(), r.stderr


def test_the_decode_runs_on_the_workers_device(tmp_path):
    """`--devices 0` names the one device; `--device` then names none (here: one the box does not have).  The file is decoded
    where the workers run, not on `--device`."""
    s = synth.synth(74, CELLS, usa=False, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s)
    closed, _ = both_doors(tmp_path, d, tg, "cr-like", ["--devices", "0", "--device", "63"])
    assert len(closed["alevin/quants_mat_rows.txt"].split()) == len(CELLS)


def test_a_decoded_file_that_does_not_fit_is_refused_with_the_sizes(tmp_path):
    """no silent fall back to the host decoder: AFQ_ERR_OOM (-7) and the sizes, before any launch, and no output directory"""
    s = synth.synth(75, CELLS, usa=False, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s)
    out = tmp_path / "out"
    r = subprocess.run([CLI, "quant", "-i", str(d), "-m", tg, "-o", str(out), "-r", "cr-like", "--sz-on-device"], capture_output=True, text=True,
                       env={**os.environ, "AFQ_TEST_SNAPPY_DEC_ROOM_BYTES": "50000"})
    assert r.returncode != 0 and "(-7)" in r.stderr and "map.collated.rad.sz: afq_snappy_frame_decode_device: the stream does not fit the device" in r.stderr, r.stderr
    assert "> 50000 bytes free" in r.stderr and not out.exists(), r.stderr


def test_a_prelude_that_is_wrong_is_refused_with_the_closed_door_s_sentence(tmp_path):
    """a reference count beyond the whole file: the same sentence from both doors (the open one does not decode on for it)"""
    s = synth.synth(76, CELLS, usa=False, **SYNTH)
    d = tmp_path / "in"
    tg, stream, first_chunk = quant_dir(d, s)
    body = bytearray(ss_decode(stream))
    body[1:9] = (1 << 40).to_bytes(8, "little")
    (d / "map.collated.rad.sz").write_bytes(rad.snappy_frame_encode(bytes(body), chunk=7000))
    errs = []
    for door in ([], ["--sz-on-device"]):
        r = subprocess.run([CLI, "quant", "-i", str(d), "-m", tg, "-o", str(tmp_path / "out"), "-r", "cr-like"] + door, capture_output=True, text=True)
        assert r.returncode != 0 and not (tmp_path / "out").exists()
        errs.append(r.stderr.strip().splitlines()[-1])
    assert errs[0] == errs[1] and "RAD header: bad ref_count" in errs[0], errs


def ss_decode(stream):
    import snappy_judge as sj

    return sj.decode(stream).data
