"""generate-permit-list, restated in plain Python from the reference's text: src/cellfilter.rs:740-780, 1686-1830 (record filter,
histogram, retained set), src/barcode_correction.rs (neighbourhoods, resolve, the compilations), src/knee_finding.rs.  Ints,
dicts and floats only; nothing from the package or the oracle is imported here.  Every function has one outcome per input."""
import math

U64 = (1 << 64) - 1
EXACT, CORRECTED, AMBIGUOUS, NOT_FOUND = "exact", "corrected", "ambiguous", "not_found"
HAMMING, SHIFT = "hamming-1", "substitution-or-shift-1"


# ---- the record pass (cellfilter.rs:1698-1771, 1775-1794) ----
def record_is_compatible(fw_bits, expected_ori):
    """fw_bits: one bool per alignment of the record (True = forward, bit 31 of the word).  `both`: always; `fw`: any
    forward; `rc`: any reverse; no alignment: only under `both`."""
    if expected_ori in ("both", "either"):
        return True
    if expected_ori == "fw":
        return any(fw_bits)
    if expected_ori == "rc":
        return any(not f for f in fw_bits)
    raise ValueError(expected_ori)


def histogram(chunks, expected_ori):
    """chunks: lists of records (bc, umi, [(ref, fw), ...]).  Returns (hist {bc: count}, n_records, n_compatible, max_ambig);
    max_ambig is the largest na among the COMPATIBLE records only."""
    hist, n_rec, n_compat, max_ambig = {}, 0, 0, 0
    for recs in chunks:
        for bc, _umi, alns in recs:
            n_rec += 1
            if record_is_compatible([bool(fw) for _r, fw in alns], expected_ori):
                n_compat += 1
                max_ambig = max(max_ambig, len(alns))
                hist[bc] = hist.get(bc, 0) + 1
    return hist, n_rec, n_compat, max_ambig


# ---- neighbourhoods (barcode_correction.rs:738-825) ----
def base_mask(n):
    return U64 if n == 32 else (1 << (2 * n)) - 1


def substitutions(bc, L):
    out = []
    for pos in range(L):
        sh = 2 * pos
        base = (bc >> sh) & 3
        cleared = bc & ~(3 << sh) & U64
        for rep in range(4):
            if rep != base:
                out.append(cleared | (rep << sh))
    return out


def shift_neighbors(bc, L):
    """for_each_shift_neighbor: what a SOURCE generates."""
    out = []
    for boundary in range(1, L):
        lower_mask = (1 << (2 * boundary)) - 1
        upper, lower = bc & ~lower_mask & U64, bc & lower_mask
        for admitted in range(4):
            insertion = upper | (admitted << (2 * (boundary - 1))) | (lower >> 2)
            deletion = (upper | admitted | ((lower & ~(3 << (2 * boundary))) << 2)) & U64
            if insertion != bc:
                out.append(insertion)
            if deletion != bc:
                out.append(deletion)
    return out


def inverse_shift_candidates(obs, L):
    """for_each_inverse_shift_candidate: the sources that would generate `obs` (repeats and `obs` itself included)."""
    out = []
    for boundary in range(1, L):
        lower_mask, low_wo = base_mask(boundary), base_mask(boundary - 1)
        ins_fixed = (obs & ~lower_mask & U64) | ((obs & low_wo) << 2)
        for terminal in range(4):
            out.append(ins_fixed | terminal)
        above = ~base_mask(boundary + 1) & U64
        del_fixed = (obs & above) | ((obs >> 2) & low_wo)
        ob = (obs >> (2 * boundary)) & 3
        for lower in range(4):
            for upper in range(4):
                if lower | upper == ob:
                    out.append(del_fixed | (lower << (2 * (boundary - 1))) | (upper << (2 * boundary)))
    return out


def neighbors(bc, L, neighborhood):
    out = substitutions(bc, L)
    if neighborhood == SHIFT:
        out += shift_neighbors(bc, L)
    return out


def validate_barcode(bc, L):
    if L < 32 and bc >= (1 << (2 * L)):
        raise ValueError(f"packed barcode {bc} does not fit declared length {L}")


# ---- the index (barcode_correction.rs:349-719) ----
class Index:
    """sources: iterable of (source, target, exact_count).  resolution: "unique" or ("frequency", (num, den), pseudocount)."""

    def __init__(self, L, neighborhood, resolution, sources):
        if not 1 <= L <= 32:
            raise ValueError(f"barcode length must be between 1 and 32 (got {L})")
        if resolution != "unique":
            _, (num, den), pseudo = resolution
            if pseudo == 0:
                raise ValueError("frequency correction requires a non-zero pseudocount")
            if den == 0 or num > den:
                raise ValueError("confidence must be between zero and one")
        self.L, self.neighborhood, self.resolution = L, neighborhood, resolution
        self.sources = {}
        for s, t, n in sources:
            validate_barcode(s, L)
            if s in self.sources and self.sources[s] != (t, n):
                raise ValueError(f"retained source barcode {s} was assigned conflicting canonical targets or exact counts")
            self.sources[s] = (t, n)

    def candidate_sources(self, obs):
        c = [s for s in substitutions(obs, self.L) if s in self.sources]
        if self.neighborhood == SHIFT:
            c += [s for s in inverse_shift_candidates(obs, self.L) if s in self.sources]
        return sorted(set(c))   # a source weighs once regardless of how many constructions lead to it

    def resolve(self, obs):
        """-> (decision, target or None)"""
        if obs in self.sources:
            return EXACT, self.sources[obs][0]
        cands = self.candidate_sources(obs)
        if self.resolution == "unique":
            targets = {self.sources[s][0] for s in cands}
            if len(targets) > 1:
                return AMBIGUOUS, None
            return (CORRECTED, next(iter(targets))) if targets else (NOT_FOUND, None)
        if not cands:
            return NOT_FOUND, None
        _, (num, den), pseudo = self.resolution
        weights = {}
        for s in cands:
            t, n = self.sources[s]
            weights[t] = weights.get(t, 0) + n + pseudo
        total = sum(weights.values())
        winner_w, winner = max((w, t) for t, w in weights.items())
        # winner / total >= num / den, exactly (Python ints do not overflow)
        return (CORRECTED, winner) if winner_w * den >= num * total else (AMBIGUOUS, None)

    @staticmethod
    def _tally(stats, decision, count):
        stats[decision + "_distinct"] += 1
        stats[decision + "_reads"] += count

    @staticmethod
    def new_stats():
        return {f"{d}_{k}": 0 for d in (EXACT, CORRECTED, AMBIGUOUS, NOT_FOUND) for k in ("distinct", "reads")}

    def compile_observed(self, observations):
        """observations: iterable of (barcode, count), repeats summed; retained identities always included.  -> (entries, stats)"""
        counts = {}
        for b, n in observations:
            counts[b] = counts.get(b, 0) + n
        for s in self.sources:
            counts.setdefault(s, 0)
        entries, stats = [], self.new_stats()
        for b in sorted(counts):
            d, t = self.resolve(b)
            self._tally(stats, d, counts[b])
            if t is not None:
                entries.append((b, t))
        return entries, stats

    def compile_distinct_observed_with_target_counts(self, observations):
        """observations: distinct (barcode, count).  -> (entries sorted by barcode, stats, target_counts {target: reads}).  A retained
        source that was never observed gets its identity entry and counts in exact_distinct, and is absent from target_counts."""
        entries, stats, tc = {}, self.new_stats(), {}
        for b, n in observations:
            d, t = self.resolve(b)
            self._tally(stats, d, n)
            if t is not None:
                entries[b] = t
                tc[t] = tc.get(t, 0) + n
        for s, (t, _n) in self.sources.items():
            if s not in entries:
                entries[s] = t
                stats["exact_distinct"] += 1
        return sorted(entries.items()), stats, tc

    def theoretical_observations(self):
        out = set()
        for s in self.sources:
            out.add(s)
            out.update(neighbors(s, self.L, self.neighborhood))
        return sorted(out)

    def compile_full_neighborhood(self):
        return self.compile_observed((b, 0) for b in self.theoretical_observations())


def identity_index(L, neighborhood, resolution, retained_counts):
    """GPL's index: every retained barcode is its own canonical target.  retained_counts: {barcode: exact count}."""
    return Index(L, neighborhood, resolution, [(b, b, n) for b, n in retained_counts.items()])


# ---- the retained set (cellfilter.rs:740-780, knee_finding.rs) ----
def rust_round(x):
    """f64::round: half away from zero (Python's round() goes to even)."""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def _distance_to_line(p1, p2, q):
    (x1, y1), (x2, y2), (x0, y0) = p1, p2, q
    numer = abs((y2 - y1) * x0 - (x2 - x1) * y0 + x2 * y1 - y2 * x1)
    a, b = (y2 - y1), (x2 - x1)
    denom = math.sqrt(a * a + b * b)
    assert denom > 0.0
    return numer / denom


def max_distance_index(cfreq):
    if len(cfreq) < 2:
        raise ValueError(f"ERROR: when attempting to find a knee-distance threshold, the list of putative cells is only of length {len(cfreq)}. "
                         "Cannot proceed. Please check the mapping rate.")
    max_x, max_y = float(len(cfreq)), float(cfreq[-1])
    p1, p2 = (0.0, float(cfreq[0]) / max_y), (1.0, float(cfreq[-1]) / max_y)
    max_d, max_ind = -1.0, 0
    for ind, f in enumerate(cfreq):
        d = _distance_to_line(p1, p2, (float(ind) / max_x, float(f) / max_y))
        if d >= max_d:
            max_d, max_ind = d, ind
    return max_ind


def get_knee(freq, max_iterations=100):
    """freq: descending.  Raises ValueError where the reference panics."""
    zero = "get_knee determined a knee index of 0. This probably should not happen with valid input data."
    cfreq, acc = [], 0
    for f in freq:
        acc += f
        cfreq.append(acc)
    prev_max, max_idx = 0, max_distance_index(cfreq)
    if max_idx == 0:
        raise ValueError(zero)
    iterations = 0
    while max_idx - prev_max != 0:
        prev_max = max_idx
        iterations += 1
        if iterations > max_iterations:
            break
        last_idx = min(len(cfreq) - 1, max_idx * 5)
        max_idx = max_distance_index(cfreq[:last_idx])
        if max_idx == 0:
            raise ValueError(zero)
    return max_idx


def select_retained(hist, method, arg=None, min_reads=10):
    """method: "knee", ("force", N) as method="force", arg=N, "expect", "unfiltered" (threshold min_reads).  hist: {bc: count}.
    -> sorted retained barcodes.  (The explicit list does not look at the histogram: the caller sorts and dedups the file.)"""
    if not hist:
        return []
    freqs = sorted(hist.values(), reverse=True)
    if method == "unfiltered":
        thr = min_reads
    elif method == "knee":
        thr = freqs[min(get_knee(freqs), len(freqs) - 1)]
    elif method == "force":
        if arg == 0:
            return []
        thr = freqs[min(max(arg - 1, 0), len(freqs) - 1)]
    elif method == "expect":
        ri = min(int(rust_round(float(arg) * 0.99)), len(freqs) - 1)
        thr = max(1, int(rust_round(float(freqs[ri]) / 10.0)))
    else:
        raise ValueError(method)
    return sorted(b for b, n in hist.items() if n >= thr)


# ---- the whole sub-command: the contents of the five files as Python maps (cellfilter.rs:369-651) ----
def parse_barcode_list(text, unfiltered, L):
    """-u: every line has one length (else ValueError), a line that is not one full valid k-mer contributes nothing.  -b: the first
    valid L-mer of every line, ValueError without one.  Lines end at \\n or \\r\\n.  -> barcodes in file order."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
    out, first = [], None
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for line in lines:
        if line.endswith("\r"):
            line = line[:-1]
        k = L
        if unfiltered:
            if first is None:
                first = len(line)
            elif len(line) != first:
                raise ValueError(f"found barcodes of different lengths {first} and {len(line)}")
            k = len(line)
        found = None
        for s in range(0, len(line) - k + 1):
            w = line[s:s + k]
            if k >= 1 and all(ch in code for ch in w):
                found = 0
                for ch in w:
                    found = (found << 2) | code[ch]
                break
        if found is not None:
            out.append(found)
        elif not unfiltered:
            raise ValueError("can't extract kmer")
    return out


def gpl_outputs(chunks, ori, method, L, arg=None, listed=None, min_reads=10, neighborhood=None, resolution="unique"):
    """method: "knee" / "expect" / "force" (arg = N), "valid_bc" (listed = the file's barcodes), "unfiltered" (listed, min_reads).
    -> dict: permit_freq, all_freq (None for unfiltered), permit_map, plan (list of (observed, corrected) ascending), stats,
    max_ambig, permit_list_type, neighborhood (the resolved one)."""
    hist, _n_rec, _n_compat, max_ambig = histogram(chunks, ori)
    filtered = method != "unfiltered"
    if method == "valid_bc":
        retained = sorted(set(listed))
    elif method == "unfiltered":
        if min_reads < 1:
            raise ValueError("min-reads < 1 is not supported")
        retained = sorted(b for b in set(listed) if hist.get(b, 0) >= min_reads)
    else:
        retained = select_retained(hist, method, arg)
    nbh = neighborhood or (SHIFT if filtered else HAMMING)   # prog_opts.rs:135-144
    idx = identity_index(L, nbh, resolution, {b: hist.get(b, 0) for b in retained})
    entries, stats, tc = idx.compile_distinct_observed_with_target_counts(sorted(hist.items()))
    plan = [(o, t) for o, t in entries if t in tc]
    if filtered:
        full, _ = idx.compile_full_neighborhood()
        permit_map = {o: t for o, t in full if t in tc}
    else:
        permit_map = dict(plan)
    return {"permit_freq": tc, "all_freq": dict(hist) if filtered else None, "permit_map": permit_map, "plan": plan, "stats": stats, "max_ambig": max_ambig,
            "permit_list_type": "filtered" if filtered else "unfiltered", "neighborhood": nbh}
