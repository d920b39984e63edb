"""`atac generate-permit-list`, restated in plain Python from the text of src/atac/cellfilter.rs of the reference alone
(initialize_rec_list :39-54, update_barcode_hist_unfiltered :68-103, populate_unfiltered_barcode_map :105-140, process_unfiltered
:143-302, generate_permit_list :304-599).  Ints, dicts and one numpy.float32 (the f32 ceiling); nothing of the package is imported.
The correction itself (CorrectionIndex and its compilations) is the restatement of tests/gpl_judge.py, imported and not copied.

Chunks are lists of records (bc, [(ref, type, start_pos, frag_len), ...])."""
import numpy as np

from gpl_judge import HAMMING, identity_index, neighbors, parse_barcode_list  # noqa: F401  (neighbors: for the cases that build barcodes a distance apart)

SIZE_RANGE = 100000   # cellfilter.rs:313
ATAC_CONFIDENCE = (9, 10)   # Confidence::ATAC


class ReferencePanics(Exception):
    """where the reference indexes past an array, or unwraps nothing"""


def bin_lens(ref_lengths, size_range=SIZE_RANGE):
    """initialize_rec_list: b_lens[r + 1] = b_lens[r] + ((ref_len as f32) / (size_range as f32)).ceil() as u64"""
    out = [0]
    for n in ref_lengths:
        q = np.float32(n) / np.float32(size_range)
        assert q.dtype == np.float32
        out.append(out[-1] + int(np.ceil(q)))
    return out


def reverse_complement(km, k):
    """needletail::bitkmer::reverse_complement of a k-mer packed first base highest, A C G T = 0 1 2 3"""
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (km & 3))
        km >>= 2
    return out


def listed_barcodes(text, rc):
    """populate_unfiltered_barcode_map: the keys of the map (a line without a full valid k-mer adds none; lines of different lengths
    are the reference's assert, a ValueError here with its words).  -> (sorted keys, the first line's length)"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    first = len(lines[0].rstrip("\r")) if lines else 0
    kms = parse_barcode_list(text, True, 0)
    if rc:
        kms = [reverse_complement(b, first) for b in kms]
    return sorted(set(kms)), first


def record_pass(chunks, blens, size_range=SIZE_RANGE):
    """update_barcode_hist_unfiltered over all chunks.  -> (hist {bc: count} over ALL records, bins, max_ambig, n_records); raises
    ReferencePanics where blens[ref] or bins[ind] is an index out of range."""
    hist, bins, max_ambig, n = {}, [0] * blens[-1], 0, 0
    for recs in chunks:
        for bc, alns in recs:
            n += 1
            max_ambig = max(max_ambig, len(alns))
            hist[bc] = hist.get(bc, 0) + 1
            if len(alns) == 1:
                ref, _ty, sp, _fl = alns[0]
                if ref >= len(blens):          # blens[ref_id as usize] (blens has ref_count + 1 entries: ref == ref_count reads the total,
                    raise ReferencePanics(f"blens[{ref}]")   # and the bin index that follows is then out of range)
                ind = blens[ref] + sp // size_range
                if ind >= len(bins):
                    raise ReferencePanics(f"bins[{ind}]")
                bins[ind] += 1
    return hist, bins, max_ambig, n


def outputs(chunks, list_text, rc, min_reads, ref_lengths, barcode_len, neighborhood=HAMMING, resolution="unique"):
    """The whole sub-command.  resolution: "unique" or "frequency" (ATAC confidence 9/10, pseudocount 1) or the explicit
    ("frequency", (num, den), 1).  -> dict: hist, bin_lens, bins, max_ambig, max_bin, n_records, listed, retained, permit_freq {target:
    reads}, plan [(observed, corrected)] ascending (permit_map.bin holds the same pairs), stats (the eight CorrectionStats)."""
    if min_reads < 1:
        raise ValueError("min-reads < 1 is not supported")
    if resolution == "frequency":
        resolution = ("frequency", ATAC_CONFIDENCE, 1)
    listed, _first = listed_barcodes(list_text, rc)
    blens = bin_lens(ref_lengths)
    hist, bins, max_ambig, n_records = record_pass(chunks, blens)
    if not bins:
        raise ReferencePanics("bins should not be empty")
    # process_unfiltered: observed_counts = every barcode with a count (listed ones with count > 0, and the unmatched); kept = listed
    # with count >= min_freq; every kept barcode is its own target with its exact count
    retained = [b for b in listed if hist.get(b, 0) >= min_reads]
    idx = identity_index(barcode_len, neighborhood, resolution, {b: hist.get(b, 0) for b in retained})
    entries, stats, tc = idx.compile_distinct_observed_with_target_counts(sorted(hist.items()))
    plan = [(o, t) for o, t in entries if t in tc]
    return {"hist": hist, "bin_lens": blens, "bins": bins, "max_ambig": max_ambig, "max_bin": max(bins), "n_records": n_records, "listed": listed,
            "retained": retained, "permit_freq": tc, "plan": plan, "stats": stats}
