"""Lifting a small synthetic workload to the top of the id spaces the library accepts, without changing what it computes.

lift_genes spreads the G genes of a SynthRad over a gene space of G_big (up to 2^20 gene ids, 1 572 864 columns under USA) by an
order-preserving affine map: gene k becomes k * stride + offset with the highest gene at G_big - 1.  Gene order, the S / U
siblings of a gene and every label stay what they were, so quantifying the lifted workload gives the rows of the small one with
the columns relabelled - bit for bit, cell_ptr, flags and values included (tests/test_id_lift_cpu.py holds the oracle to it).
lift_refs shifts every ref id up by ref_base and pads tid_to_gid in front; the rows do not change at all.

The records are the small workload's: a lifted run costs what the small run costs, plus whatever the code under test spends on
the size of the id space - which is the point."""
import dataclasses

import numpy as np

from util import pkg

SIZES = [30000, 9000, 4000, 1500, 700, 260, 250, 120, 99, 40, 3]   # the workload of tests/test_gpu_em.py: about 46 k reads
SMALL_GENES = 400
TOP_CELL_READS = 150   # (above small_thresh: the cell is not on the tiny-cell path)


def workload(usa, seed=5):
    """The EM tests' workload, and behind it one cell that guarantees the LAST output column under every resolution: reads of
    the highest gene alone - under USA with its spliced and its unspliced ref, so that they count in the ambiguous section, the
    last column of the matrix (the Zipf-skewed cells name the highest gene a few times, but not under every resolution with
    that status)."""
    s = pkg.synth.synth(seed, SIZES, num_genes=SMALL_GENES, txp_per_gene=3, usa=usa, dup=0.5, zipf=0.6, cross=0.4, umi_err=0.02,
                        max_extra_na=5)
    n = TOP_CELL_READS
    top_s, top_u = 3 * SMALL_GENES - 1, 3 * SMALL_GENES + SMALL_GENES - 1   # last spliced txp; (USA) the last gene's unspliced ref
    refs = np.tile(np.asarray([top_s, top_u] if usa else [top_s], np.uint32), n)
    umi = pkg.synth.splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(77)) & np.uint64((1 << 24) - 1)
    return dataclasses.replace(s, cell_nrec=np.append(s.cell_nrec, n), cell_bc=np.append(s.cell_bc, np.uint64(0xFFFFFFF1)),
                               umi=np.concatenate((s.umi, umi)), na=np.append(s.na, np.full(n, 2 if usa else 1, np.int64)),
                               refs=np.concatenate((s.refs, refs)))


@dataclasses.dataclass
class GeneLift:
    s: object             # the lifted SynthRad: same records, new tid_to_gid / num_genes / num_rows
    gene_map: np.ndarray  # [G] gene index k -> k'
    gid_map: np.ndarray   # [small num_genes] gene id -> lifted gene id (USA: 2k+s -> 2k'+s; otherwise the gene map)
    col_map: np.ndarray   # [small num_rows] output column -> lifted column (USA: section * G_big + k')

    def relabel(self, res, resolution):
        """The QuantResult of the small workload as the lifted workload must give it.  `trivial` under USA counts per gene id
        (trivial_counts indexes [0, num_genes)): the gid map; everything else per output column - the cells below small_thresh
        under `trivial` as well, which take the tiny-cell rule whatever the resolution."""
        old = np.asarray(res.gene, np.int64)
        new = self.col_map[np.minimum(old, len(self.col_map) - 1)]
        if self.s.usa and resolution == "trivial":
            tiny = (np.asarray(res.flags) & pkg._abi.CELL_TINY_PATH) != 0
            by_gid = np.repeat(~tiny, np.diff(res.cell_ptr.astype(np.int64)))
            new = np.where(by_gid, self.gid_map[np.minimum(old, len(self.gid_map) - 1)], new)
        return dataclasses.replace(res, gene=new.astype(np.uint32), cell_ptr=np.array(res.cell_ptr), val=np.array(res.val))


def lift_genes(s, G_big):
    """G_big: genes of the lifted workload (its num_genes is G_big, under USA 2 * G_big and its num_rows 3 * G_big)."""
    G = s.num_genes // 2 if s.usa else s.num_genes
    assert G >= 2 and G_big >= G
    stride = (G_big - 1) // (G - 1)
    offset = G_big - 1 - (G - 1) * stride
    gene_map = np.arange(G, dtype=np.int64) * stride + offset
    assert gene_map[-1] == G_big - 1 and np.all(np.diff(gene_map) > 0)
    if s.usa:
        gid = np.arange(2 * G, dtype=np.int64)
        gid_map = 2 * gene_map[gid >> 1] + (gid & 1)
        col = np.arange(3 * G, dtype=np.int64)
        col_map = (col // G) * G_big + gene_map[col % G]
        num_genes, num_rows = 2 * G_big, 3 * G_big
    else:
        gid_map = col_map = gene_map
        num_genes = num_rows = G_big
    t2g = gid_map[s.tid_to_gid.astype(np.int64)].astype(np.uint32)
    lifted = dataclasses.replace(s, tid_to_gid=t2g, num_genes=num_genes, num_rows=num_rows)
    return GeneLift(lifted, gene_map, gid_map, col_map)


def lift_refs(s, ref_base):
    """Every ref id up by ref_base; tid_to_gid padded in front with gene 0, which no record names any more."""
    t2g = np.zeros(ref_base + len(s.tid_to_gid), dtype=np.uint32)
    t2g[ref_base:] = s.tid_to_gid
    refs = (s.refs.astype(np.uint64) + np.uint64(ref_base))
    assert int(refs.max()) < (1 << 31)
    return dataclasses.replace(s, refs=refs.astype(np.uint32), tid_to_gid=t2g)
