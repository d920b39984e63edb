"""Multi-barcode generate-permit-list, restated in plain Python from the reference's text: src/cellfilter.rs:110-366 (routes,
per-sample output), 789-1381 (do_generate_permit_list_multi_bc), 1405-1682 (sample list, sample permit map), src/prog_opts.rs:47-184
(modes and specs), src/correction_plan.rs:23-172 (the plan's layout), src/barcode_correction.rs:479-484, 612-629 (the structural
table).  The index, the retained set, the barcode lists and the record filter are tests/gpl_judge.py's, by import.  Ints, dicts and
strings only; nothing from the package is imported here.  Every function has one outcome per input."""
import math

import gpl_judge as J

HAMMING, SHIFT = J.HAMMING, J.SHIFT
RNA_CONF = (39, 40)
SAMPLE_MODES = ("exact", "unique", "frequency", "1-edit")
MODE_DEBUG = {"exact": "Exact", "unique": "Unique", "frequency": "Frequency", "1-edit": "OneEdit"}   # format!("{:?}", SampleCorrectionMode)
ORI_SYMBOL = {"both": "both", "either": "both", "fw": "fw", "rc": "rc"}   # the spelling the package's single-barcode generate_permit_list.json uses
TIMING_AND_SIZE_KEYS = ("cell_correction_seconds", "correction_plan_bytes", "correction_plan_write_seconds")   # sample_info.json, top level
ROUTING_TIMING_KEYS = ("replay_seconds",)                                                                       # ... under sample_routing


# ---- the record pass as the device sees it: routing entries in, (entry, cell) pairs out ----
def pair_histogram(chunks, entries, expected_ori):
    """chunks: lists of records (b0, b1, umi, [(ref, fw), ...]); entries: ascending distinct sample barcodes.  A compatible record
    (has_alignment_on_strand, cellfilter.rs:974 - gpl_judge.record_is_compatible) whose b0 is entries[e] counts the pair (e, b1); any
    other compatible record is unrouted.  -> ({(e, b1): count}, stats)"""
    assert list(entries) == sorted(set(entries))
    pos = {b: i for i, b in enumerate(entries)}
    pairs, st = {}, {"n_records": 0, "n_compatible": 0, "n_routed": 0, "n_unrouted": 0}
    for recs in chunks:
        for b0, b1, _umi, alns in recs:
            st["n_records"] += 1
            if not J.record_is_compatible([bool(fw) for _r, fw in alns], expected_ori):
                continue
            st["n_compatible"] += 1
            e = pos.get(b0)
            if e is None:
                st["n_unrouted"] += 1
            else:
                st["n_routed"] += 1
                pairs[(e, b1)] = pairs.get((e, b1), 0) + 1
    return pairs, st


# ---- the sample list (cellfilter.rs:1405-1569) ----
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
_RC = {"A": "T", "T": "A", "C": "G", "G": "C", "a": "t", "t": "a", "c": "g", "g": "c"}


def pack(seq):
    """the whole sequence as one k-mer, first base highest (BitNuclKmer::new(seq, len, false).next())"""
    if not seq or any(ch not in _CODE for ch in seq):
        raise ValueError(f"couldn't pack sample barcode: {seq}")
    v = 0
    for ch in seq:
        v = (v << 2) | _CODE[ch]
    return v


def load_sample_list(text, reverse=False):
    """-> {"canonical": [canonical barcodes in order of first appearance], "rotations": {observed: canonical},
    "names": {canonical: name}, "L": bases}.  One column: the barcode is its own sample and name; two: barcode, name; three or more:
    observed, canonical, name.  ValueError with the reference's sentence where it bails."""
    rot, names, order, L = {}, {}, [], None
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for line in lines:
        if line.endswith("\r"):
            line = line[:-1]
        t = line.strip()
        if not t or t.startswith("#"):
            continue
        parts = t.split("\t")
        if len(parts) >= 3:
            obs, canon, name = parts[0], parts[1], parts[2]
        elif len(parts) == 2:
            obs, canon, name = parts[0], parts[0], parts[1]
        else:
            obs, canon, name = parts[0], parts[0], parts[0]
        if len(obs.encode()) != len(canon.encode()):
            raise ValueError(f"sample barcode '{obs}' and its canonical barcode '{canon}' have different lengths")
        n = len(obs.encode())
        if not 1 <= n <= 32:
            raise ValueError(f"sample barcode length {n} is unsupported; expected 1 through 32 bases")
        if L is not None and L != n:
            raise ValueError(f"sample barcode file mixes lengths {L} and {n}")
        L = n
        if reverse:
            obs, canon = ("".join(_RC.get(ch, ch) for ch in reversed(s)) for s in (obs, canon))
        po, pc = pack(obs), pack(canon)
        if rot.get(po, pc) != pc:
            raise ValueError(f"sample construction barcode '{obs}' is assigned to conflicting canonical barcodes")
        rot[po] = pc
        if names.get(pc, name) != name:
            raise ValueError(f"canonical sample barcode '{canon}' is assigned conflicting names '{names[pc]}' and '{name}'")
        if pc not in names:
            order.append(pc)
            names[pc] = name
    if L is None:
        raise ValueError("sample barcode list contains no barcodes")
    return {"canonical": order, "rotations": rot, "names": names, "L": L}


# ---- specs (prog_opts.rs:135-184) ----
def _reduced(c):
    """Confidence::new (barcode_correction.rs:79-90) reduces by the gcd (a gcd of 0 counts as 1)"""
    g = math.gcd(c[0], c[1]) or 1
    return c[0] // g, c[1] // g


def sample_spec(mode, neighborhood=HAMMING, confidence=RNA_CONF):
    """-> None (exact) or (neighborhood, resolution)"""
    if mode == "exact":
        return None
    if mode == "unique":
        return neighborhood, "unique"
    if mode == "frequency":
        return neighborhood, ("frequency", _reduced(confidence), 1)
    if mode == "1-edit":
        return SHIFT, "unique"
    raise ValueError(mode)


def cell_spec(correction="unique", neighborhood=None, confidence=RNA_CONF):
    """resolved_cell_neighborhood(true): hamming-1 unless given"""
    return neighborhood or HAMMING, ("unique" if correction == "unique" else ("frequency", _reduced(confidence), 1))


# ---- routing (build_sample_permit_map, cellfilter.rs:1581-1666; compile_structural_neighborhood) ----
def structural_table(info, neighborhood):
    """-> (entries {barcode: target} with exactly one structurally possible target, ambiguous [barcodes] with more)"""
    topo = J.Index(info["L"], neighborhood, "unique", [(s, t, 0) for s, t in info["rotations"].items()])
    entries, ambiguous = {}, []
    for b in topo.theoretical_observations():
        d, t = topo.resolve(b)   # (Unique resolution IS structural_resolution: exact, else unique_neighbor_target)
        if t is not None:
            entries[b] = t
        elif d == J.AMBIGUOUS:
            ambiguous.append(b)
    return entries, ambiguous


def build_routing(info, spec):
    """-> {"permit_map": {observed: canonical} as the record pass uses it, "deferred": sorted barcodes whose decision waits for the
    exact counts (Frequency only), "entries": the ascending union - what the device call gets as sample_observed}"""
    permit_map, deferred = dict(info["rotations"]), []
    if spec is not None:
        entries, ambiguous = structural_table(info, spec[0])
        permit_map.update(entries)
        if spec[1] != "unique":
            deferred = sorted(ambiguous)
    assert not set(deferred) & set(permit_map)
    return {"permit_map": permit_map, "deferred": deferred, "entries": sorted(set(permit_map) | set(deferred))}


# ---- the whole pass up to the per-sample histograms (cellfilter.rs:863-1190) ----
def route_pairs(info, spec, routing, pairs, n_records, n_unrouted, whitelist=None):
    """pairs: {(entry index, cell): count} over routing["entries"].  -> per-sample exact / unmatched histograms, the final sample
    permit map, the totals and the sample_routing tallies."""
    idx_of = {c: i for i, c in enumerate(info["canonical"])}
    ns = len(info["canonical"])
    hist, unmatched = [dict() for _ in range(ns)], [dict() for _ in range(ns)]
    ent = routing["entries"]
    per_entry = {}
    for (e, cell), n in pairs.items():
        per_entry.setdefault(ent[e], {})[cell] = n
    tally = {"exact": 0, "structurally_unique": 0, "immediate_rejected": n_unrouted, "deferred": 0, "deferred_accepted": 0, "deferred_rejected": 0}

    def add(sample, cells):
        for cell, n in cells.items():
            dst = hist[sample] if whitelist is None or cell in whitelist else unmatched[sample]
            dst[cell] = dst.get(cell, 0) + n

    exact_counts = {}
    for b, cells in per_entry.items():
        reads = sum(cells.values())
        if b in routing["permit_map"]:
            if b in info["rotations"]:
                tally["exact"] += reads
                exact_counts[b] = reads
            else:
                tally["structurally_unique"] += reads
            add(idx_of[routing["permit_map"][b]], cells)
        else:
            tally["deferred"] += reads
    permit_map = dict(routing["permit_map"])
    if spec is not None and spec[1] != "unique":
        fidx = J.Index(info["L"], spec[0], spec[1], [(s, t, exact_counts.get(s, 0)) for s, t in info["rotations"].items()])
        permit_map = dict(fidx.compile_full_neighborhood()[0])
        for b in routing["deferred"]:
            cells = per_entry.get(b)
            if not cells:
                continue
            _d, t = fidx.resolve(b)
            if t is not None:
                tally["deferred_accepted"] += sum(cells.values())
                add(idx_of[t], cells)
            else:
                tally["deferred_rejected"] += sum(cells.values())
    matched = tally["exact"] + tally["structurally_unique"] + tally["deferred_accepted"]
    return {"hist": hist, "unmatched": unmatched, "sample_permit_map": permit_map, "tally": tally, "total_reads": n_records, "matched_reads": matched,
            "unmatched_reads": tally["immediate_rejected"] + tally["deferred_rejected"]}


# ---- one sample (compile_multi_sample_cell_output, cellfilter.rs:193-366) ----
def sample_output(name, sample_bc, cell_hist, unmatched, cspec, method, L, arg=None, listed=None, min_reads=0):
    """method: "knee" / "expect" / "force" (arg), "valid_bc" (listed: the -b file's barcodes), "unfiltered" (min_reads; the whitelist
    split cell_hist from unmatched already).  -> {"info", "permit_map", "permit_freq", "plan"}; the two maps are None for an empty sample."""
    if not cell_hist:
        return {"info": {"name": name, "barcode": f"0x{sample_bc:x}", "num_reads": 0, "num_cells": 0, "collatable_reads": 0, "cell_correction": J.Index.new_stats()},
                "permit_map": None, "permit_freq": None, "plan": []}
    if method == "valid_bc":
        kept = sorted(set(listed))
    elif method == "unfiltered":
        kept = J.select_retained(cell_hist, "unfiltered", min_reads=min_reads)
    else:
        kept = J.select_retained(cell_hist, method, arg)
    observed = dict(cell_hist)
    for b, n in unmatched.items():
        observed[b] = observed.get(b, 0) + n
    exact_retained = sum(observed.get(b, 0) for b in kept)
    idx = J.identity_index(L, cspec[0], cspec[1], {b: observed.get(b, 0) for b in kept})
    entries, stats, tc = idx.compile_distinct_observed_with_target_counts(sorted(observed.items()))
    legacy = entries if method == "unfiltered" else idx.compile_full_neighborhood()[0]
    collatable = sum(tc.values())
    return {"info": {"name": name, "barcode": f"0x{sample_bc:x}", "num_reads": collatable if method == "unfiltered" else exact_retained, "num_cells": len(tc),
                     "collatable_reads": collatable, "cell_correction": stats},
            "permit_map": {o: t for o, t in legacy if t in tc}, "permit_freq": tc, "plan": [(o, t) for o, t in entries if t in tc]}


# ---- correction_plan.bin (correction_plan.rs:23-45, 132-161; bincode: u64 lengths, u32 variants, Option as a tag byte) ----
def _u(v, n):
    return int(v).to_bytes(n, "little")


def _spec_bytes(L, spec):
    nbh, res = spec
    out = bytes([L]) + _u({HAMMING: 0, SHIFT: 1}[nbh], 4)
    if res == "unique":
        return out + _u(0, 4)
    _, (num, den), pseudo = res
    return out + _u(1, 4) + _u(num, 8) + _u(den, 8) + _u(pseudo, 8)


def _pairs_bytes(pairs):
    pairs = sorted(pairs)
    return _u(len(pairs), 8) + b"".join(_u(o, 8) + _u(c, 8) for o, c in pairs)


def plan_bytes(sample_L, cell_L, sspec, sample_corrections, cspec, scopes):
    """scopes: (canonical sample barcode, [(observed, corrected)]); written in ascending sample-barcode order (write_to sorts)"""
    out = b"AFCORR\0\0" + _u(1, 2) + bytes([1, sample_L, cell_L])
    out += b"\x00" if sspec is None else b"\x01" + _spec_bytes(sample_L, sspec)
    out += _pairs_bytes(sample_corrections.items())
    scopes = sorted(scopes)
    out += _u(len(scopes), 8)
    for sb, pp in scopes:
        out += b"\x01" + _u(sb, 8) + _spec_bytes(cell_L, cspec) + _pairs_bytes(pp)
    return out


# ---- the whole step: the contents of every file as Python values ----
def filter_debug(method, arg=None, list_file=None, min_reads=0):
    """format!("{:?}", CellFilterMethod) for paths without a quote or a backslash"""
    return {"knee": "KneeFinding", "expect": f"ExpectCells({arg})", "force": f"ForceCells({arg})", "valid_bc": f'ExplicitList("{list_file}")',
            "unfiltered": f'UnfilteredExternalList("{list_file}", {min_reads})'}[method]


def gpl_multi_outputs(chunks, ori, sample_text, cell_L, method, arg=None, listed=None, min_reads=0, list_file=None, sample_mode="exact",
                      sample_neighborhood=HAMMING, sample_confidence=RNA_CONF, reverse=False, cell_correction="unique", cell_neighborhood=None,
                      cell_confidence=RNA_CONF, cmdline="", num_barcodes=2):
    """chunks of (b0, b1, umi, alns) records.  listed: the barcodes of the -b file (valid_bc) or of the -u whitelist (unfiltered).
    -> {"sample_permit_map", "samples": [(dir name, permit_map or None, permit_freq or None)], "plan": bytes, "sample_info",
    "generate_permit_list"} - the two JSON documents without their timing and byte-size keys."""
    info = load_sample_list(sample_text, reverse)
    sspec = sample_spec(sample_mode, sample_neighborhood, sample_confidence)
    cspec = cell_spec(cell_correction, cell_neighborhood, cell_confidence)
    routing = build_routing(info, sspec)
    pairs, st = pair_histogram(chunks, routing["entries"], ori)
    whitelist = set(listed) if method == "unfiltered" else None
    r = route_pairs(info, sspec, routing, pairs, st["n_records"], st["n_unrouted"], whitelist)
    samples, infos, scopes, total_cells = [], [], [], 0
    for i, canon in enumerate(info["canonical"]):
        name = info["names"][canon]
        o = sample_output(name, canon, r["hist"][i], r["unmatched"][i], cspec, method, cell_L, arg=arg, listed=listed, min_reads=min_reads)
        samples.append((f"sample_{name}", o["permit_map"], o["permit_freq"]))
        infos.append(o["info"])
        scopes.append((canon, o["plan"]))
        total_cells += o["info"]["num_cells"]
    conf = lambda c: "%d/%d" % _reduced(c)
    resolved = {"exact": "exact", "unique": "unique", "1-edit": "unique", "frequency": "frequency"}[sample_mode]
    common = {"cell_bc_correction": cell_correction, "cell_bc_neighborhood": cspec[0], "cell_bc_confidence": conf(cell_confidence),
              "sample_bc_correction": resolved, "sample_bc_neighborhood": None if sspec is None else sspec[0], "sample_bc_confidence": conf(sample_confidence)}
    routing_json = dict(r["tally"], spill_runs=0, spill_pairs_after_run_length_encoding=0, spill_compressed_bytes=0, spill_uncompressed_bytes=0)
    sample_info = dict({"num_samples": len(info["canonical"]), "num_barcodes": num_barcodes, "total_cells": total_cells, "total_reads": r["total_reads"],
                        "matched_reads": r["matched_reads"], "unmatched_reads": r["unmatched_reads"], "sample_correction_mode": MODE_DEBUG[sample_mode],
                        "sample_bc_ori": "Reverse" if reverse else "Forward", "sample_routing": routing_json, "samples": infos}, **common)
    meta = dict({"velo_mode": False, "expected_ori": ORI_SYMBOL[ori], "version_str": "0.18.0", "cmd": cmdline,
                 "permit-list-type": filter_debug(method, arg, list_file, min_reads), "multi_barcode": True, "num_barcodes": num_barcodes}, **common)
    return {"sample_permit_map": r["sample_permit_map"], "samples": samples, "plan": plan_bytes(info["L"], cell_L, sspec, r["sample_permit_map"], cspec, scopes),
            "sample_info": sample_info, "generate_permit_list": meta, "total_cells": total_cells, "routing": routing, "routed": r, "stats": st}


def strip_measured(sample_info):
    """sample_info.json without the keys that hold what a run measured"""
    out = {k: v for k, v in sample_info.items() if k not in TIMING_AND_SIZE_KEYS}
    out["sample_routing"] = {k: v for k, v in sample_info["sample_routing"].items() if k not in ROUTING_TIMING_KEYS}
    return out
