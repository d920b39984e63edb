"""Host-side mirror of the reference's per-cell quant interface, over the C ABI.

The reference is compiled Rust whose hot path has no plugin/FFI surface: it is
called from `run_worker_thread` (src/quant.rs:659-1325) and configured by
`WorkerConfig` (src/quant.rs:398-416).  `WorkerConfig` below carries the same
fields with the same meaning; `Quantifier.quant_chunks` takes collated chunk
bytes (one chunk = one cell) and returns the rows the worker would have emitted.

There is no CPU fallback: if csrc/libafquant.so (hand-written HIP for gfx950) is
missing or no device is usable, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import AfqBatchStats, AfqBootstraps, AfqConfig, AfqEqclasses, AfqKernelTime, AfqResult, RESOLUTIONS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AFQ_LIB_PATH") or os.path.join(_HERE, "csrc", "libafquant.so")   # (AFQ_LIB_PATH: a measurement build, profiles/ only)


class AfqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"afquant error {code}: {msg}")
        self.code = code


@dataclass
class WorkerConfig:
    """Field-for-field WorkerConfig (src/quant.rs:398-416) + record field widths."""

    resolution: str = "cr-like"
    usa_mode: bool = False
    num_genes: int = 0  # gene-id space of tid_to_gid (USA: 2*G)
    num_rows: int = 0  # output columns (USA: 3*G)
    small_thresh: int = 100  # tiny_cell_thresh, DEFAULT_SMALL_CELL_FAST_THRESHOLD quant.rs:449
    large_graph_thresh: int = 0  # main.rs:332-341: 1000 for parsimony*, else 0
    pug_exact_umi: bool = True  # main.rs:652-703: umi-edit-dist 0 unless parsimony*
    sa_model: str = "winner-take-all"
    em_init_uniform: bool = False
    bc_bytes: int = 4
    umi_bytes: int = 4
    bc_split: int = 0  # multi-barcode records of unequal widths: bytes of b0, the first of the two integers in the bc_bytes field (0: one integer)
    umi_len: int = 0  # UMI length in bases if known (RAD file tag ulen); 0 = unknown
    dump_eq: bool = False  # -d: keep each cell's gene-level equivalence classes (QuantResult.eqclasses; -em resolutions)
    num_bootstraps: int = 0  # -b: bootstrap replicates per non-tiny cell (QuantResult.bootstraps; -em resolutions)
    summary_stat: bool = False  # --summary-stat: population variance of the replicates instead of the n-1 sample variance
    boot_seed: int = 0  # key of the counter-based generator behind the bootstrap draws
    profile: bool = False

    @staticmethod
    def for_resolution(resolution: str, **kw) -> "WorkerConfig":
        """Apply the CLI's conditional defaults (src/main.rs:320-341, 652-703)."""
        pars = resolution.startswith("parsimony")
        d = dict(resolution=resolution, large_graph_thresh=1000 if pars else 0, pug_exact_umi=not pars)
        d.update(kw)
        return WorkerConfig(**d)

    def to_c(self) -> AfqConfig:
        if self.resolution not in RESOLUTIONS:
            raise ValueError(f"unknown resolution {self.resolution!r}")
        c = AfqConfig()
        c.abi_version = _abi.AFQ_ABI_VERSION
        c.resolution = RESOLUTIONS[self.resolution]
        c.sa_model = {"winner-take-all": 0, "prefer-ambig": 1}[self.sa_model]
        c.usa_mode = int(self.usa_mode)
        c.num_genes = self.num_genes
        c.num_rows = self.num_rows
        c.small_thresh = self.small_thresh
        c.large_graph_thresh = self.large_graph_thresh
        c.pug_exact_umi = int(self.pug_exact_umi)
        c.em_init_uniform = int(self.em_init_uniform)
        c.bc_bytes = self.bc_bytes
        c.umi_bytes = self.umi_bytes
        c.bc_split = int(self.bc_split)
        c.profile = int(self.profile)
        c.umi_len = int(self.umi_len)
        c.dump_eq = 1 if self.dump_eq else 0
        c.num_bootstraps = int(self.num_bootstraps)
        c.summary_stat = 1 if self.summary_stat else 0
        c.boot_seed = int(self.boot_seed)
        return c


@dataclass
class QuantResult:
    """Rows for a run of cells: CSR of (output column, f32 count) + per-cell scalars."""

    first_cell_index: int
    cell_ptr: np.ndarray
    gene: np.ndarray
    val: np.ndarray
    bc: np.ndarray
    nrec: np.ndarray
    flags: np.ndarray

    @property
    def n_cells(self) -> int:
        return len(self.bc)

    def row(self, i: int):
        a, b = int(self.cell_ptr[i]), int(self.cell_ptr[i + 1])
        return self.gene[a:b], self.val[a:b]

    def cell_stats(self, i: int):
        """sum/max/num_expr/mean_by_max/num_genes_over_mean as src/quant.rs:1150-1196."""
        _, v = self.row(i)
        s = np.float32(0.0)
        for x in v:  # f32 sum in gene-index order
            s = np.float32(s + x)
        mx = np.float32(v.max()) if len(v) else np.float32(0)
        n = len(v)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.float32(s) / np.float32(n)
            over = int((v > mean).sum())
            return dict(sum_umi=float(s), max_umi=float(mx), num_expr=n, mean_by_max=float(mean / mx),
                        num_genes_over_mean=over, dedup_rate=float(s / np.float32(self.nrec[i])))


@dataclass
class EqClasses:
    """-d: per-cell gene-level equivalence classes (label = ascending gene ids, count = molecules), CSR over CSR."""

    cell_ptr: np.ndarray
    label_ptr: np.ndarray
    labels: np.ndarray
    count: np.ndarray

    def cell(self, i: int):
        """Classes of cell i as a sorted list of (label tuple, count) - the reference's order is a hash map's."""
        a, b = int(self.cell_ptr[i]), int(self.cell_ptr[i + 1])
        lp = self.label_ptr
        return sorted((tuple(int(x) for x in self.labels[int(lp[k]):int(lp[k + 1])]), int(self.count[k])) for k in range(a, b))


@dataclass
class Bootstraps:
    """-b: per-cell non-zero bootstrap means and variances (two CSR matrices; columns = gene ids of gene_eqc's labels)."""

    mean_ptr: np.ndarray
    mean_col: np.ndarray
    mean_val: np.ndarray
    var_ptr: np.ndarray
    var_col: np.ndarray
    var_val: np.ndarray

    def mean(self, i: int):
        a, b = int(self.mean_ptr[i]), int(self.mean_ptr[i + 1])
        return self.mean_col[a:b], self.mean_val[a:b]

    def var(self, i: int):
        a, b = int(self.var_ptr[i]), int(self.var_ptr[i + 1])
        return self.var_col[a:b], self.var_val[a:b]


def bootstraps_from_c(bs) -> Bootstraps:
    def arr(ptr, count, dt):
        return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dt, copy=True) if count else np.zeros(0, dtype=dt)

    n = int(bs.n_cells)
    mp, vp = arr(bs.mean_ptr, n + 1, np.uint64), arr(bs.var_ptr, n + 1, np.uint64)
    nm, nv = int(mp[-1]), int(vp[-1])
    return Bootstraps(mp, arr(bs.mean_col, nm, np.uint32), arr(bs.mean_val, nm, np.float32), vp, arr(bs.var_col, nv, np.uint32),
                      arr(bs.var_val, nv, np.float32))


def eqclasses_from_c(ec) -> EqClasses:
    def arr(ptr, count, dt):
        return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dt, copy=True) if count else np.zeros(0, dtype=dt)

    n, k, w = int(ec.n_cells), int(ec.n_classes), int(ec.n_words)
    return EqClasses(arr(ec.cell_ptr, n + 1, np.uint64), arr(ec.label_ptr, k + 1, np.uint64), arr(ec.labels, w, np.uint32),
                     arr(ec.count, k, np.uint32))


class _ResultOwner:
    """Keeps a library-owned afq_result alive while numpy views point into it."""

    def __init__(self, release, res: AfqResult):
        self._release, self._res = release, res

    def __del__(self):
        try:
            self._release(C.byref(self._res))
        except Exception:
            pass


def result_from_c(res: AfqResult, owner=None) -> QuantResult:
    """With `owner` the big CSR arrays are zero-copy views of the library's pinned buffers
    (the owner releases them when the QuantResult is garbage collected); without, everything is copied."""
    n, nnz = int(res.n_cells), int(res.nnz)

    def arr(ptr, count, dt, view=False):
        if count == 0:
            return np.zeros(0, dtype=dt)
        a = np.ctypeslib.as_array(ptr, shape=(count,))
        return a if view else a.astype(dt, copy=True)

    z = owner is not None
    out = QuantResult(int(res.first_cell_index), arr(res.cell_ptr, n + 1, np.uint64), arr(res.gene, nnz, np.uint32, z),
                      arr(res.val, nnz, np.float32, z), arr(res.bc, n, np.uint64), arr(res.nrec, n, np.uint32),
                      arr(res.flags, n, np.uint8))
    out._owner = owner
    return out


_lib = None


def configure_runtime():
    """Runtime settings the path wants, set while they can still take effect: GPU_FORCE_BLIT_COPY_SIZE=0 (device<->host copies on
    the DMA engines, not as blit kernels on the compute queue next to the path's own kernels) is read by the HIP runtime when it
    comes up, so it is set here only when NO HIP runtime is mapped into the process yet (torch not imported, libamdhip64 not
    loaded) and the host has not said otherwise.  A host whose runtime is already up keeps its own setting; afq_create notes a
    missing one on stderr.  Returns True when the setting is in place."""
    import sys

    if "GPU_FORCE_BLIT_COPY_SIZE" in os.environ:
        return os.environ["GPU_FORCE_BLIT_COPY_SIZE"] == "0"
    mapped = "torch" in sys.modules
    if not mapped:
        try:
            with open("/proc/self/maps") as f:
                mapped = "libamdhip64" in f.read()
        except OSError:
            mapped = False
    if mapped:
        return False
    os.environ["GPU_FORCE_BLIT_COPY_SIZE"] = "0"
    return True


def load_library(path: str = LIB_PATH):
    """dlopen the HIP library and declare prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # libafquant.so needs libamdhip64.so.7.  PyTorch-ROCm bundles its own copy under the same
    # soname; a process must hold exactly one HIP/HSA runtime, so when torch is installed it is
    # imported first and the library binds to the runtime torch already mapped (a torch-free
    # host gets /opt/rocm's).  See DESIGN.md "one HIP runtime per process".
    # (GPU_FORCE_BLIT_COPY_SIZE=0 - copies on the DMA engines, not as blit kernels next to the path's own - must be in the environment
    #  before the HIP runtime comes up: bench.py, the afquant CLI and tests/conftest.py set it; configure_runtime() sets it for a Python
    #  host that imports this binding before any HIP runtime is mapped and has not chosen a value itself.  afq_create says so once on
    #  stderr when it is missing.  INTEGRATION.md "runtime settings")
    configure_runtime()
    try:
        import torch  # noqa: F401

        if torch.cuda.is_available():
            torch.cuda.init()   # torch brings its HIP runtime up first; initialising it AFTER this library has used HIP finds no GPU
    except ImportError:
        pass
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: the HIP extension is not built (run __graft_entry__.build()). "
            "There is no CPU fallback for the quant hot path."
        )
    lib = C.CDLL(path)
    p = C.POINTER
    lib.afq_create.argtypes = [p(AfqConfig), p(C.c_uint32), C.c_uint32, C.c_int, p(C.c_void_p)]
    lib.afq_create.restype = C.c_int
    lib.afq_destroy.argtypes = [C.c_void_p]
    lib.afq_destroy.restype = None
    lib.afq_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint64]
    lib.afq_submit.restype = C.c_int
    lib.afq_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint64]
    lib.afq_submit_device.restype = C.c_int
    lib.afq_set_aln_extra_bytes.argtypes = [C.c_void_p, C.c_uint32]
    lib.afq_set_aln_extra_bytes.restype = C.c_int
    lib.afq_collect.argtypes = [C.c_void_p, p(AfqResult)]
    lib.afq_collect.restype = C.c_int
    lib.afq_result_release.argtypes = [p(AfqResult)]
    lib.afq_result_release.restype = None
    lib.afq_result_eqclasses.argtypes = [p(AfqResult), p(AfqEqclasses)]
    lib.afq_result_eqclasses.restype = C.c_int
    lib.afq_result_bootstraps.argtypes = [p(AfqResult), p(AfqBootstraps)]
    lib.afq_result_bootstraps.restype = C.c_int
    lib.afq_infer.argtypes = [C.c_void_p, p(C.c_uint32), p(C.c_uint64), C.c_uint32, p(C.c_uint64), p(C.c_uint32), p(C.c_uint32), C.c_uint32,
                              C.c_uint32, C.c_uint32, p(AfqResult)]
    lib.afq_infer.restype = C.c_int
    lib.afq_atac_dedup.argtypes = [C.c_void_p, p(C.c_uint32), p(C.c_uint32), p(C.c_uint16), p(C.c_uint64), C.c_uint32,
                                   p(p(C.c_uint64)), p(p(C.c_uint32)), p(p(C.c_uint32)), p(p(C.c_uint16)), p(p(C.c_uint16))]
    lib.afq_atac_dedup.restype = C.c_int
    lib.afq_atac_dedup_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_int, p(p(C.c_uint64)),
                                       p(p(C.c_uint64)), p(p(C.c_uint32)), p(p(C.c_uint32)), p(p(C.c_uint16)), p(p(C.c_uint16)), p(_abi.AfqAtacStats)]
    lib.afq_atac_dedup_rad.restype = C.c_int
    lib.afq_atac_sort_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_int, p(C.c_uint64), p(C.c_uint64),
                                      C.c_uint64, p(C.c_uint32), C.c_uint32, p(C.c_uint64), p(p(C.c_uint32)), p(p(C.c_uint32)), p(p(C.c_uint16)),
                                      p(p(C.c_uint64)), p(p(C.c_uint32)), p(_abi.AfqAtacSortStats)]
    lib.afq_atac_sort_rad.restype = C.c_int
    lib.afq_atac_sort_limits.argtypes = [p(C.c_uint32)]
    lib.afq_atac_sort_limits.restype = None
    lib.afq_atac_sort_leaf_limits.argtypes = [p(C.c_uint32)]
    lib.afq_atac_sort_leaf_limits.restype = None
    lib.afq_atac_sort_table_slot.argtypes = [C.c_uint64, C.c_uint64, p(C.c_uint32), p(C.c_uint32)]
    lib.afq_atac_sort_table_slot.restype = None
    lib.afq_gpl_hist_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                     p(C.c_uint64), p(p(C.c_uint64)), p(p(C.c_uint64)), p(_abi.AfqGplHistStats)]
    lib.afq_gpl_hist_rad.restype = C.c_int
    lib.afq_gpl_correct.argtypes = [C.c_void_p, p(C.c_uint64), p(C.c_uint64), C.c_uint64, p(C.c_uint64), p(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, p(p(C.c_uint8)), p(p(C.c_uint32)), p(p(C.c_uint64)),
                                    p(_abi.AfqGplCorrectionStats)]
    lib.afq_gpl_correct.restype = C.c_int
    lib.afq_gpl_limits.argtypes = [p(C.c_uint32)]
    lib.afq_gpl_limits.restype = None
    lib.afq_gpl_table_slot.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, p(C.c_uint32), p(C.c_uint32)]
    lib.afq_gpl_table_slot.restype = None
    lib.afq_atac_gpl_hist_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_int, p(C.c_uint64), C.c_uint32,
                                          C.c_uint32, p(C.c_uint64), p(p(C.c_uint64)), p(p(C.c_uint64)), p(p(C.c_uint64)), p(_abi.AfqAtacGplHistStats)]
    lib.afq_atac_gpl_hist_rad.restype = C.c_int
    lib.afq_atac_gpl_limits.argtypes = [p(C.c_uint32)]
    lib.afq_atac_gpl_limits.restype = None
    lib.afq_gpl_multi_hist_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                           p(C.c_uint64), C.c_uint64, p(C.c_uint64), p(p(C.c_uint32)), p(p(C.c_uint64)), p(p(C.c_uint64)),
                                           p(_abi.AfqGplMultiHistStats)]
    lib.afq_gpl_multi_hist_rad.restype = C.c_int
    lib.afq_gpl_multi_limits.argtypes = [p(C.c_uint32)]
    lib.afq_gpl_multi_limits.restype = None
    lib.afq_generate_permit_list_multi.argtypes = [p(_abi.AfqGplMultiOpts)]
    lib.afq_generate_permit_list_multi.restype = C.c_int64
    lib.afq_atac_generate_permit_list.argtypes = [p(_abi.AfqAtacGplOpts)]
    lib.afq_atac_generate_permit_list.restype = C.c_int
    lib.afq_host_last_error.argtypes = []
    lib.afq_host_last_error.restype = C.c_char_p
    lib.afq_collate_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                    p(C.c_uint64), p(C.c_uint64), C.c_uint64, p(C.c_uint64), C.c_uint64, p(p(C.c_uint8)), p(C.c_uint64), p(p(C.c_uint64)),
                                    p(p(C.c_uint32)), p(_abi.AfqCollateStats)]
    lib.afq_collate_rad.restype = C.c_int
    lib.afq_collate_limits.argtypes = [p(C.c_uint32)]
    lib.afq_collate_limits.restype = None
    lib.afq_collate_multi_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                          p(C.c_uint64), p(C.c_uint32), C.c_uint64, p(C.c_uint32), p(C.c_uint64), p(C.c_uint64), C.c_uint64, p(C.c_uint32),
                                          p(C.c_uint64), C.c_uint64, p(C.c_uint32), C.c_uint64, p(p(C.c_uint8)), p(C.c_uint64), p(p(C.c_uint64)),
                                          p(p(C.c_uint32)), p(_abi.AfqCollateMultiStats)]
    lib.afq_collate_multi_rad.restype = C.c_int
    lib.afq_collate_multi_limits.argtypes = [p(C.c_uint32)]
    lib.afq_collate_multi_limits.restype = None
    lib.afq_collate_multi.argtypes = [p(_abi.AfqCollateMultiOpts)]
    lib.afq_collate_multi.restype = C.c_int
    # (afq_collate, afq_atac_collate and the three _sz doors: _collate_dirs declares them on function objects of its own)
    lib.afq_snappy_frame_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, p(p(C.c_uint8)), p(C.c_uint64), p(_abi.AfqSnappyStats)]
    lib.afq_snappy_frame_encode.restype = C.c_int
    lib.afq_snappy_limits.argtypes = [p(C.c_uint32)]
    lib.afq_snappy_limits.restype = None
    lib.afq_snappy_frame_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, p(p(C.c_uint8)), p(C.c_uint64), p(_abi.AfqSnappyStats)]
    lib.afq_snappy_frame_decode_device.restype = C.c_int
    lib.afq_collated_chunk_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, p(p(C.c_uint64)), p(p(C.c_uint32)), p(p(C.c_uint32)),
                                             p(p(C.c_uint64)), p(C.c_uint64)]
    lib.afq_collated_chunk_table.restype = C.c_int
    lib.afq_snappy_decode_limits.argtypes = [p(C.c_uint32)]
    lib.afq_snappy_decode_limits.restype = None
    lib.afq_set_collate_compress.argtypes = [C.c_void_p, C.c_int]
    lib.afq_set_collate_compress.restype = None
    lib.afq_atac_collate_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_int, p(C.c_uint64), p(C.c_uint64),
                                         C.c_uint64, p(C.c_uint64), C.c_uint64, p(p(C.c_uint8)), p(C.c_uint64), p(C.c_uint64), p(p(C.c_uint64)),
                                         p(p(C.c_uint32)), p(p(C.c_uint32)), p(_abi.AfqAtacCollateStats)]
    lib.afq_atac_collate_rad.restype = C.c_int
    lib.afq_atac_collate_limits.argtypes = [p(C.c_uint32)]
    lib.afq_atac_collate_limits.restype = None
    lib.afq_convert_bam_rad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, p(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                        p(p(C.c_uint8)), p(C.c_uint64), p(p(C.c_uint64)), p(p(C.c_uint32)), p(C.c_uint64), p(_abi.AfqConvertStats)]
    lib.afq_convert_bam_rad.restype = C.c_int
    lib.afq_convert_limits.argtypes = [p(C.c_uint32)]
    lib.afq_convert_limits.restype = None
    lib.afq_convert.argtypes = [p(_abi.AfqConvertOpts)]
    lib.afq_convert.restype = C.c_int
    lib.afq_convert_with.argtypes = [p(_abi.AfqConvertOpts), C.c_uint32]
    lib.afq_convert_with.restype = C.c_int
    lib.afq_bgzf_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, p(p(C.c_uint8)), p(C.c_uint64), p(_abi.AfqInflateStats)]
    lib.afq_bgzf_inflate_device.restype = C.c_int
    lib.afq_inflate_limits.argtypes = [p(C.c_uint32)]
    lib.afq_inflate_limits.restype = None
    lib.afq_convert_prelude_bytes.argtypes = [p(C.c_char_p), C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
    lib.afq_convert_prelude_bytes.restype = C.c_int64
    lib.afq_view_file.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    lib.afq_view_file.restype = C.c_int
    lib.afq_free.argtypes = [C.c_void_p]
    lib.afq_free.restype = None
    lib.afq_get_kernel_times.argtypes = [C.c_void_p, p(AfqKernelTime), C.c_uint32]
    lib.afq_get_kernel_times.restype = C.c_int
    lib.afq_get_batch_stats.argtypes = [C.c_void_p, p(AfqBatchStats)]
    lib.afq_get_batch_stats.restype = C.c_int
    lib.afq_last_error.argtypes = [C.c_void_p]
    lib.afq_last_error.restype = C.c_char_p
    lib.afq_abi_version.argtypes = []
    lib.afq_abi_version.restype = C.c_int
    if lib.afq_abi_version() != _abi.AFQ_ABI_VERSION:
        raise RuntimeError("libafquant.so ABI version mismatch")
    _lib = lib
    return lib


def atac_sort_limits():
    """afq_atac_sort_limits and afq_atac_sort_leaf_limits: {"bin_shift", "leaf_cap", "repartition_above", "parse_tile", "small_leaf",
    "small_leaf_threads", "leaf_threads", "parse_halo"} of the `atac sort` kernels."""
    out, leaf = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    load_library().afq_atac_sort_limits(out)
    load_library().afq_atac_sort_leaf_limits(leaf)
    return {"bin_shift": int(out[0]), "leaf_cap": int(out[1]), "repartition_above": int(out[2]), "parse_tile": int(out[3]),
            "small_leaf": int(leaf[0]), "small_leaf_threads": int(leaf[1]), "leaf_threads": int(leaf[2]), "parse_halo": int(leaf[3])}


def atac_sort_table_slot(barcode, n_corr):
    """afq_atac_sort_table_slot: (home slot of `barcode`, capacity) of the correction table afq_atac_sort_rad builds for n_corr entries."""
    slot, cap = C.c_uint32(), C.c_uint32()
    load_library().afq_atac_sort_table_slot(int(barcode), int(n_corr), C.byref(slot), C.byref(cap))
    return int(slot.value), int(cap.value)


def gpl_limits():
    """afq_gpl_limits: {"parse_tile", "parse_halo", "lane_alns"} of the generate-permit-list parse - bytes staged per trip, bytes
    staged behind them, and the alignment count above which a record is a long record."""
    out = (C.c_uint32 * 4)()
    load_library().afq_gpl_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "lane_alns": int(out[2])}


def collate_limits():
    """afq_collate_limits: {"parse_tile", "parse_halo", "lane_alns", "radix_block"} of collate - bytes a walk stages per trip, bytes
    staged behind them, the alignment count above which the whole wave handles a record, keys a workgroup of a radix pass takes."""
    out = (C.c_uint32 * 4)()
    load_library().afq_collate_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "lane_alns": int(out[2]), "radix_block": int(out[3])}


def collate_multi_limits():
    """afq_collate_multi_limits: collate_limits' four values for multi-barcode collate (the walks are collate's over another head, the
    placement is collate's own).  Tests build their edge shapes from these."""
    out = (C.c_uint32 * 4)()
    load_library().afq_collate_multi_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "lane_alns": int(out[2]), "radix_block": int(out[3])}


def _collate_dirs(plain, sz, opts_t, stats_t, input_dir, rad_dir, compress, device, cmdline):
    lib = load_library()
    st = stats_t()
    o = opts_t()
    o.input_dir, o.rad_dir, o.device, o.cmdline = os.fsencode(input_dir), os.fsencode(rad_dir), int(device), cmdline.encode()
    o.stats_out = C.pointer(st)
    fn = lib[sz if compress else plain]   # (a function object of this call's own: a host may have declared the symbol's prototype over its own struct type)
    fn.argtypes, fn.restype = [C.POINTER(opts_t)], C.c_int
    rc = fn(C.byref(o))
    if rc:
        raise AfqError(int(rc), (lib.afq_host_last_error() or b"").decode())
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def collate_multi(input_dir, rad_dir, device: int = 0, cmdline: str = "", compress: bool = False):
    """afq_collate_multi: multi-barcode `collate` - the output directory of generate_permit_list_multi and the mapper's directory in;
    map.collated.rad, collation_manifest.bin, collate.json and unmapped_bc_count_collated.bin are written into input_dir.  compress:
    afq_collate_multi_sz - map.collated.rad.sz (snappy frame streams, compressed on the device) in place of map.collated.rad, and
    collate.json says so.  Returns the device call's stats; raises AfqError."""
    return _collate_dirs("afq_collate_multi", "afq_collate_multi_sz", _abi.AfqCollateMultiOpts, _abi.AfqCollateMultiStats, input_dir, rad_dir, compress, device, cmdline)


def collate(input_dir, rad_dir, compress: bool = False, device: int = 0, cmdline: str = ""):
    """afq_collate: `collate` - the output directory of generate-permit-list and the mapper's directory in; map.collated.rad,
    collate.json and unmapped_bc_count_collated.bin are written into input_dir.  compress: afq_collate_sz - map.collated.rad.sz
    (snappy frame streams, compressed on the device) in place of map.collated.rad, and collate.json says so.  Returns the device
    call's stats; raises AfqError."""
    return _collate_dirs("afq_collate", "afq_collate_sz", _abi.AfqCollateOpts, _abi.AfqCollateStats, input_dir, rad_dir, compress, device, cmdline)


def atac_collate(input_dir, rad_dir, compress: bool = False, device: int = 0, cmdline: str = ""):
    """afq_atac_collate: `atac collate`, as collate() for a scATAC RAD (compress: afq_atac_collate_sz)."""
    return _collate_dirs("afq_atac_collate", "afq_atac_collate_sz", _abi.AfqAtacCollateOpts, _abi.AfqAtacCollateStats, input_dir, rad_dir, compress, device, cmdline)


def snappy_limits():
    """afq_snappy_limits: {"block", "hash_slots", "max_copy", "blocks_per_workgroup"} of the device snappy frame encoder - bytes of
    input per frame chunk, slots of a chunk's last-position table, the longest single copy element, chunks a workgroup takes."""
    out = (C.c_uint32 * 4)()
    load_library().afq_snappy_limits(out)
    return {"block": int(out[0]), "hash_slots": int(out[1]), "max_copy": int(out[2]), "blocks_per_workgroup": int(out[3])}


def snappy_decode_limits():
    """afq_snappy_decode_limits: {"window", "threads", "piece_chunks", "lds_bytes"} of the device snappy frame decoder - bytes of a chunk's
    body staged per trip, threads of a workgroup (it takes one data chunk), data chunks of one launch at the most, LDS bytes of a workgroup."""
    out = (C.c_uint32 * 4)()
    load_library().afq_snappy_decode_limits(out)
    return {"window": int(out[0]), "threads": int(out[1]), "piece_chunks": int(out[2]), "lds_bytes": int(out[3])}


def inflate_limits():
    """afq_inflate_limits: {"threads", "piece_blocks", "lds_bytes", "blocks_per_workgroup"} of the device BGZF inflater - threads of a
    workgroup, BGZF blocks of one launch at the most, LDS bytes of a workgroup, blocks a workgroup takes."""
    out = (C.c_uint32 * 4)()
    load_library().afq_inflate_limits(out)
    return {"threads": int(out[0]), "piece_blocks": int(out[1]), "lds_bytes": int(out[2]), "blocks_per_workgroup": int(out[3])}


def convert_limits():
    """afq_convert_limits: {"parse_tile", "parse_halo", "lane_alns", "scan_block"} of convert - bytes of a span a walk stages per trip,
    bytes staged behind them, the record count above which the whole wave takes a run, flags a workgroup of the run-number and rank scans takes."""
    out = (C.c_uint32 * 4)()
    load_library().afq_convert_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "lane_alns": int(out[2]), "scan_block": int(out[3])}


def convert(bam, rad_out, filter_best: bool = False, num_threads: int = 8, device: int = 0, inflate_on_device: bool = False):
    """afq_convert_with: `convert` - the BAM `bam` (CR / UR tags on its records) as the mapper RAD `rad_out`.  inflate_on_device: the
    BGZF blocks are inflated on the device (`--inflate-on-device`) instead of on host threads; the file written and the stats do
    not depend on it.  Returns the device call's stats; raises AfqError."""
    lib = load_library()
    st = _abi.AfqConvertStats()
    o = _abi.AfqConvertOpts()
    o.bam, o.rad_out, o.num_threads, o.filter_best, o.device = os.fsencode(bam), os.fsencode(rad_out), int(num_threads), int(bool(filter_best)), int(device)
    o.stats_out = C.pointer(st)
    rc = lib.afq_convert_with(C.byref(o), _abi.AFQ_CONVERT_INFLATE_ON_DEVICE if inflate_on_device else 0)
    if rc:
        raise AfqError(int(rc), (lib.afq_host_last_error() or b"").decode())
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def convert_prelude(ref_names, num_chunks: int, cblen: int, ulen: int) -> bytes:
    """afq_convert_prelude_bytes: the prelude `convert` writes for these reference names, chunk count and lengths."""
    lib = load_library()
    names = (C.c_char_p * max(len(ref_names), 1))(*[n.encode() for n in ref_names])
    n = lib.afq_convert_prelude_bytes(names, len(ref_names), int(num_chunks), int(cblen), int(ulen), None, 0)
    if n < 0:
        raise AfqError(int(n), (lib.afq_host_last_error() or b"").decode())
    buf = (C.c_uint8 * max(int(n), 1))()
    lib.afq_convert_prelude_bytes(names, len(ref_names), int(num_chunks), int(cblen), int(ulen), buf, int(n))
    return bytes(buf[: int(n)])


def view(rad, header: bool = False) -> str:
    """afq_view_file: `view` - the records of the RAD file as text, one line per alignment (the reference names first with `header`)."""
    import tempfile

    lib = load_library()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "view.txt")
        rc = lib.afq_view_file(os.fsencode(rad), int(bool(header)), os.fsencode(out))
        if rc:
            raise AfqError(int(rc), (lib.afq_host_last_error() or b"").decode())
        with open(out) as f:
            return f.read()


def atac_collate_limits():
    """afq_atac_collate_limits: {"parse_tile", "parse_halo", "aln_bytes", "radix_block"} of `atac collate` - bytes a walk stages per
    trip, bytes staged behind them, bytes of an alignment, keys a workgroup of a radix pass takes."""
    out = (C.c_uint32 * 4)()
    load_library().afq_atac_collate_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "aln_bytes": int(out[2]), "radix_block": int(out[3])}


def gpl_multi_limits():
    """afq_gpl_multi_limits: {"parse_tile", "parse_halo", "lane_alns"} of the multi-barcode generate-permit-list parse - bytes staged per
    trip, bytes staged behind them, and the number of alignments above which a record is tested by the whole wave.  Tests build their
    edge shapes from these."""
    out = (C.c_uint32 * 4)()
    load_library().afq_gpl_multi_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "lane_alns": int(out[2])}


def atac_gpl_limits():
    """afq_atac_gpl_limits: {"parse_tile", "parse_halo", "private_bins"} of the `atac generate-permit-list` record pass - bytes a walk
    stages per trip, bytes staged behind them, bins a workgroup counts privately in LDS (0: the bins are counted in global memory)."""
    out = (C.c_uint32 * 4)()
    load_library().afq_atac_gpl_limits(out)
    return {"parse_tile": int(out[0]), "parse_halo": int(out[1]), "private_bins": int(out[2])}


def atac_generate_permit_list(input_dir, output_dir, list_file, min_reads: int = 10, rc: bool = True, num_threads: int = 8, correction="unique",
                              neighborhood="hamming-1", confidence=(0, 0), device: int = 0, fill_bytes: int = 0, cmdline: str = ""):
    """afq_atac_generate_permit_list: the whole `atac generate-permit-list` step from the mapper's directory (map.rad) and an unfiltered
    barcode list into output_dir (permit_freq.bin, permit_map.bin, correction_plan.bin, bin_recs.bin, bin_lens.bin,
    generate_permit_list.json).  confidence (0, 0) is the ATAC default 9/10.  Returns the record pass's stats as a dict; raises AfqError."""
    lib = load_library()
    st = _abi.AfqAtacGplHistStats()
    o = _abi.AfqAtacGplOpts()
    o.input_dir, o.output_dir, o.list_file = os.fsencode(input_dir), os.fsencode(output_dir), os.fsencode(list_file)
    o.min_reads, o.rc, o.num_threads = int(min_reads), 1 if rc else 0, int(num_threads)
    o.frequency = _abi.GPL_RESOLUTIONS[correction] if isinstance(correction, str) else int(correction)
    o.neighborhood = _abi.GPL_NEIGHBORHOODS[neighborhood] if isinstance(neighborhood, str) else int(neighborhood)
    o.conf_num, o.conf_den = int(confidence[0]), int(confidence[1])
    o.device, o.fill_bytes, o.cmdline = int(device), int(fill_bytes), cmdline.encode()
    o.stats_out = C.pointer(st)
    rc_ = lib.afq_atac_generate_permit_list(C.byref(o))
    if rc_ != 0:
        raise AfqError(rc_, (lib.afq_host_last_error() or b"").decode())
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def generate_permit_list_multi(input_dir, output_dir, sample_bc_list, method="knee", method_count: int = 0, list_file=None, min_reads: int = 10,
                               expected_ori="fw", correction="unique", neighborhood=None, confidence=(0, 0), sample_correction="exact",
                               sample_neighborhood="hamming-1", sample_confidence=(0, 0), sample_bc_ori="forward", num_threads: int = 8, device: int = 0,
                               fill_bytes: int = 0, cmdline: str = ""):
    """afq_generate_permit_list_multi: the whole `generate-permit-list` step on a multi-barcode (10x Flex) RAD - the mapper's directory
    (map.rad) and the sample barcode list in, sample_permit_map.bin, sample_<name>/permit_map.bin / permit_freq.bin, correction_plan.bin,
    sample_info.json and generate_permit_list.json out.  method: "knee", "expect" / "force" (method_count), "valid_bc" / "unfiltered"
    (list_file; min_reads with "unfiltered").  sample_correction: "exact", "unique", "frequency" or the deprecated "1-edit".  A
    confidence of (0, 0) is 39/40; neighborhood None is the multi-barcode default, hamming-1.  Returns {"total_cells": ..., "stats": the
    record pass's stats}; raises AfqError."""
    lib = load_library()
    st = _abi.AfqGplMultiHistStats()
    o = _abi.AfqGplMultiOpts()
    o.input_dir, o.output_dir, o.sample_bc_list = os.fsencode(input_dir), os.fsencode(output_dir), os.fsencode(sample_bc_list)
    o.expected_ori = _abi.GPL_ORI[expected_ori.lower()] if isinstance(expected_ori, str) else int(expected_ori)
    o.method = _abi.GPL_METHODS[method] if isinstance(method, str) else int(method)
    o.method_count, o.min_reads = int(method_count), int(min_reads)
    o.list_file = None if list_file is None else os.fsencode(list_file)
    o.frequency = _abi.GPL_RESOLUTIONS[correction] if isinstance(correction, str) else int(correction)
    o.neighborhood = -1 if neighborhood is None else (_abi.GPL_NEIGHBORHOODS[neighborhood] if isinstance(neighborhood, str) else int(neighborhood))
    o.conf_num, o.conf_den = int(confidence[0]), int(confidence[1])
    o.sample_correction = _abi.GPL_SAMPLE_CORRECTIONS[sample_correction] if isinstance(sample_correction, str) else int(sample_correction)
    o.sample_neighborhood = _abi.GPL_NEIGHBORHOODS[sample_neighborhood] if isinstance(sample_neighborhood, str) else int(sample_neighborhood)
    o.sample_conf_num, o.sample_conf_den = int(sample_confidence[0]), int(sample_confidence[1])
    o.sample_bc_ori = _abi.GPL_SAMPLE_ORI[sample_bc_ori.lower()] if isinstance(sample_bc_ori, str) else int(sample_bc_ori)
    o.num_threads, o.device, o.fill_bytes, o.cmdline = int(num_threads), int(device), int(fill_bytes), cmdline.encode()
    o.stats_out = C.pointer(st)
    n = lib.afq_generate_permit_list_multi(C.byref(o))
    if n < 0:
        raise AfqError(int(n), (lib.afq_host_last_error() or b"").decode())
    return {"total_cells": int(n), "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}


def gpl_table_slot(barcode, n_kept, bc_bytes: int = 8):
    """afq_gpl_table_slot: (home slot of `barcode`, capacity) of the counting table afq_gpl_hist_rad builds for n_kept compatible records."""
    slot, cap = C.c_uint32(), C.c_uint32()
    load_library().afq_gpl_table_slot(int(barcode), int(n_kept), int(bc_bytes), C.byref(slot), C.byref(cap))
    return int(slot.value), int(cap.value)


class _Held(np.ndarray):
    """ndarray view that keeps the owner of its memory alive."""


class Quantifier:
    """One per device: config + tid_to_gid resident on the GPU (afq_ctx)."""

    def __init__(self, cfg: WorkerConfig, tid_to_gid: np.ndarray, device: int = 0, aln_extra_bytes: int = 0):
        """aln_extra_bytes: records carry a position of this many bytes (1, 2, 4, 8) behind every alignment word (the RAD
        alignment tag `pos`; afq_set_aln_extra_bytes); 0 = plain records."""
        self.lib = load_library()
        self.cfg = cfg
        self._t2g = np.ascontiguousarray(tid_to_gid, dtype=np.uint32)
        ccfg = cfg.to_c()
        h = C.c_void_p()
        rc = self.lib.afq_create(C.byref(ccfg), self._t2g.ctypes.data_as(C.POINTER(C.c_uint32)), len(self._t2g),
                                 device, C.byref(h))
        if rc != 0:
            raise AfqError(rc, (self.lib.afq_last_error(None) or b"").decode())
        self._h = h
        if aln_extra_bytes:
            self.set_aln_extra_bytes(aln_extra_bytes)

    def set_aln_extra_bytes(self, e: int):
        """Width of the position behind every alignment word of the records submitted from now on (0: none)."""
        self._check(self.lib.afq_set_aln_extra_bytes(self._h, int(e)))

    def set_collate_compress(self, on: bool):
        """afq_set_collate_compress: collate_rad, collate_multi_rad and atac_collate_rad hand "bytes" out as the snappy frame stream of the
        chunk bytes, compressed on the device; offsets, counts and stats stay in uncompressed coordinates."""
        self.lib.afq_set_collate_compress(self._h, int(bool(on)))

    def snappy_frame_encode(self, data, d_ptr: int = 0, n_bytes: int = 0):
        """afq_snappy_frame_encode: the snappy frame stream of `data` (host bytes, or d_ptr/n_bytes for bytes already on the device),
        compressed on the device.  Returns (bytes, stats)."""
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), int(n_bytes), 1
        else:
            b = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        o_b, o_n, st = C.POINTER(C.c_uint8)(), C.c_uint64(), _abi.AfqSnappyStats()
        self._check(self.lib.afq_snappy_frame_encode(self._h, ptr, nb, on_dev, C.byref(o_b), C.byref(o_n), C.byref(st)))
        try:
            return C.string_at(o_b, int(o_n.value)), {k: int(getattr(st, k)) for k, _ in st._fields_}
        finally:
            self.lib.afq_free(o_b)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.afq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise AfqError(rc, (self.lib.afq_last_error(self._h) or b"").decode())

    def submit(self, chunk_bytes, chunk_off, first_cell_index: int = 0):
        b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        self._keep = (b, off)
        self._check(self.lib.afq_submit(self._h, b.ctypes.data_as(C.c_void_p), b.nbytes,
                                        off.ctypes.data_as(C.POINTER(C.c_uint64)), len(off), first_cell_index))

    def submit_ptr(self, h_ptr: int, n_bytes: int, chunk_off, first_cell_index: int = 0):
        """afq_submit from a raw host address (e.g. pinned memory the caller owns)."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        self._keep = (off,)
        self._check(self.lib.afq_submit(self._h, C.c_void_p(h_ptr), n_bytes,
                                        off.ctypes.data_as(C.POINTER(C.c_uint64)), len(off), first_cell_index))

    def submit_device(self, d_ptr: int, n_bytes: int, chunk_off, first_cell_index: int = 0):
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        self._keep = (off,)
        self._check(self.lib.afq_submit_device(self._h, C.c_void_p(d_ptr), n_bytes,
                                               off.ctypes.data_as(C.POINTER(C.c_uint64)), len(off), first_cell_index))

    def collect(self) -> QuantResult:
        res = AfqResult()
        self._check(self.lib.afq_collect(self._h, C.byref(res)))
        out = result_from_c(res, owner=_ResultOwner(self.lib.afq_result_release, res))
        if self.cfg.dump_eq:
            ec = AfqEqclasses()
            self._check(self.lib.afq_result_eqclasses(C.byref(res), C.byref(ec)))
            out.eqclasses = eqclasses_from_c(ec)
        if self.cfg.num_bootstraps:
            bs = AfqBootstraps()
            self._check(self.lib.afq_result_bootstraps(C.byref(res), C.byref(bs)))
            out.bootstraps = bootstraps_from_c(bs)
        return out

    def infer(self, eq_labels, cell_classes, num_alphas: int, usa_mode: bool = False) -> QuantResult:
        """`alevin-fry infer` (src/infer.rs): eq_labels = list of label lists (global classes); cell_classes = per cell a list of
        (class id, count) with ascending class ids.  Returns the non-zero abundances per cell."""
        lab = np.asarray([x for l in eq_labels for x in l], dtype=np.uint32)
        lp = np.zeros(len(eq_labels) + 1, dtype=np.uint64)
        lp[1:] = np.cumsum([len(l) for l in eq_labels])
        cp = np.zeros(len(cell_classes) + 1, dtype=np.uint64)
        cp[1:] = np.cumsum([len(c) for c in cell_classes])
        ce = np.asarray([e for c in cell_classes for e, _ in c], dtype=np.uint32)
        cc = np.asarray([n for c in cell_classes for _, n in c], dtype=np.uint32)
        u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        res = AfqResult()
        self._check(self.lib.afq_infer(self._h, lab.ctypes.data_as(u32), lp.ctypes.data_as(u64), len(eq_labels), cp.ctypes.data_as(u64),
                                       ce.ctypes.data_as(u32), cc.ctypes.data_as(u32), len(cell_classes), int(num_alphas), 1 if usa_mode else 0,
                                       C.byref(res)))
        return result_from_c(res, owner=_ResultOwner(self.lib.afq_result_release, res))

    def quant_chunks(self, chunk_bytes, chunk_off, first_cell_index: int = 0) -> QuantResult:
        self.submit(chunk_bytes, chunk_off, first_cell_index)
        return self.collect()

    def snappy_frame_decode(self, stream, shift: int = 0, on_device: bool = False):
        """afq_snappy_frame_decode_device: the bytes of the snappy frame stream `stream` (host bytes), decoded on the device.  Returns
        (bytes, stats); with on_device (device pointer, n_bytes, stats) instead - decoded byte x lies at pointer + shift + x, and the
        memory is the context's, valid until the next decode on it or close()."""
        b = np.ascontiguousarray(np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream)
        o_b, o_n, st = C.POINTER(C.c_uint8)(), C.c_uint64(), _abi.AfqSnappyStats()
        self._check(self.lib.afq_snappy_frame_decode_device(self._h, b.ctypes.data_as(C.c_void_p), b.nbytes, int(shift), 1 if on_device else 0, C.byref(o_b),
                                                            C.byref(o_n), C.byref(st)))
        stats = {k: int(getattr(st, k)) for k, _ in st._fields_}
        if on_device:
            return C.cast(o_b, C.c_void_p).value or 0, int(o_n.value), stats
        try:
            return C.string_at(o_b, int(o_n.value)), stats
        finally:
            self.lib.afq_free(o_b)

    def bgzf_inflate(self, data, shift: int = 0, on_device: bool = False):
        """afq_bgzf_inflate_device: the bytes of the BGZF file `data` (host bytes), inflated on the device.  Returns (bytes, stats);
        with on_device ((device pointer, n_bytes), stats) instead - inflated byte x lies at pointer + shift + x, the pointer is
        16-byte aligned, and the memory is the context's, valid until the next inflate on it or close()."""
        b = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
        o_b, o_n, st = C.POINTER(C.c_uint8)(), C.c_uint64(), _abi.AfqInflateStats()
        self._check(self.lib.afq_bgzf_inflate_device(self._h, b.ctypes.data_as(C.c_void_p), b.nbytes, int(shift), 1 if on_device else 0, C.byref(o_b), C.byref(o_n),
                                                     C.byref(st)))
        stats = {k: int(getattr(st, k)) for k, _ in st._fields_}
        if on_device:
            return (C.cast(o_b, C.c_void_p).value or 0, int(o_n.value)), stats
        try:
            return C.string_at(o_b, int(o_n.value)), stats
        finally:
            self.lib.afq_free(o_b)

    def collated_chunk_table(self, d_ptr: int, n_bytes: int, first_chunk: int = 0, rec_hdr_bytes: int = 0):
        """afq_collated_chunk_table: the chunk table of the collated record stream of n_bytes at device pointer d_ptr, hopped on the
        device from first_chunk.  Returns (off, nbytes, nrec, first_bc) as arrays, one entry a chunk."""
        o_off, o_nb, o_nr, o_bc, o_n = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint64()
        self._check(self.lib.afq_collated_chunk_table(self._h, C.c_void_p(d_ptr), int(n_bytes), int(first_chunk), int(rec_hdr_bytes), C.byref(o_off), C.byref(o_nb),
                                                      C.byref(o_nr), C.byref(o_bc), C.byref(o_n)))
        try:
            n = int(o_n.value)
            return tuple(np.ctypeslib.as_array(a, shape=(n,)).copy() if n else np.zeros(0, t) for a, t in ((o_off, np.uint64), (o_nb, np.uint32), (o_nr, np.uint32), (o_bc, np.uint64)))
        finally:
            for a in (o_off, o_nb, o_nr, o_bc):
                self.lib.afq_free(a)

    def kernel_times(self):
        buf = (AfqKernelTime * 64)()
        n = self.lib.afq_get_kernel_times(self._h, buf, 64)
        if n < 0:
            self._check(n)
        return {buf[i].name.decode(): (buf[i].ms, buf[i].launches) for i in range(n)}

    def label_rehash_count(self) -> int:
        """Ranges of cells decoded again under another label-hash function after a collision (parsimony; see afquant.h)."""
        self.lib.afq_label_rehash_count.restype = C.c_uint64
        self.lib.afq_label_rehash_count.argtypes = [C.c_void_p]
        return int(self.lib.afq_label_rehash_count(self._h))

    def pool_regrow_count(self) -> int:
        """Ranges of cells run again with four times the parsimony pool because a cell's graph outgrew it (see afquant.h)."""
        self.lib.afq_pool_regrow_count.restype = C.c_uint64
        self.lib.afq_pool_regrow_count.argtypes = [C.c_void_p]
        return int(self.lib.afq_pool_regrow_count(self._h))

    def mono_cell_count(self) -> int:
        """Parsimony cells resolved by the one-workgroup kernel (afq_mono_cell_count)."""
        self.lib.afq_mono_cell_count.restype = C.c_uint64
        self.lib.afq_mono_cell_count.argtypes = [C.c_void_p]
        return int(self.lib.afq_mono_cell_count(self._h))

    def resolve_divert_count(self) -> int:
        """Buckets of the last batch the hash resolve handed to the sort path (afq_resolve_divert_count)."""
        self.lib.afq_resolve_divert_count.restype = C.c_uint64
        self.lib.afq_resolve_divert_count.argtypes = [C.c_void_p]
        return int(self.lib.afq_resolve_divert_count(self._h))

    def em_resize_count(self) -> int:
        """Ranges whose EM scratch had to be sized on the host (the device-side plan did not fit what was set aside)."""
        self.lib.afq_em_resize_count.restype = C.c_uint64
        self.lib.afq_em_resize_count.argtypes = [C.c_void_p]
        return int(self.lib.afq_em_resize_count(self._h))

    def em_instance_counts(self) -> list:
        """Cells of the last collected batch per rounds instance of the order-free EM (tiers 0-4), then the tier 4 cells that ran
        with 32-bit state ids (afq_em_instance_counts)."""
        out = (C.c_uint64 * 6)()
        self.lib.afq_em_instance_counts.restype = None
        self.lib.afq_em_instance_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self.lib.afq_em_instance_counts(self._h, out)
        return [int(x) for x in out]

    def range_pipeline_counts(self) -> list:
        """The last batch's ranges, those whose rows crossed on the copy stream without the host waiting, those that fell back
        to the waiting path after draining it, and the result-array growths that had to wait for rows in flight
        (afq_range_pipeline_counts)."""
        out = (C.c_uint64 * 4)()
        self.lib.afq_range_pipeline_counts.restype = None
        self.lib.afq_range_pipeline_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self.lib.afq_range_pipeline_counts(self._h, out)
        return [int(x) for x in out]

    def batch_stats(self) -> dict:
        s = AfqBatchStats()
        self._check(self.lib.afq_get_batch_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def atac_dedup(self, ref, start, frag_len, cell_ptr):
        ref = np.ascontiguousarray(ref, np.uint32)
        start = np.ascontiguousarray(start, np.uint32)
        frag_len = np.ascontiguousarray(frag_len, np.uint16)
        cell_ptr = np.ascontiguousarray(cell_ptr, np.uint64)
        n_cells = len(cell_ptr) - 1
        o_ptr, o_ref, o_start = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        o_len, o_cnt = C.POINTER(C.c_uint16)(), C.POINTER(C.c_uint16)()
        self._check(self.lib.afq_atac_dedup(
            self._h, ref.ctypes.data_as(C.POINTER(C.c_uint32)), start.ctypes.data_as(C.POINTER(C.c_uint32)),
            frag_len.ctypes.data_as(C.POINTER(C.c_uint16)), cell_ptr.ctypes.data_as(C.POINTER(C.c_uint64)), n_cells,
            C.byref(o_ptr), C.byref(o_ref), C.byref(o_start), C.byref(o_len), C.byref(o_cnt)))
        try:
            ptr = np.ctypeslib.as_array(o_ptr, shape=(n_cells + 1,)).copy()
            n = int(ptr[-1])
            mk = lambda p_, dt: (np.ctypeslib.as_array(p_, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt))
            return ptr, mk(o_ref, np.uint32), mk(o_start, np.uint32), mk(o_len, np.uint16), mk(o_cnt, np.uint16)
        finally:
            for q in (o_ptr, o_ref, o_start, o_len, o_cnt):
                self.lib.afq_free(q)

    @staticmethod
    def atac_sort_limits():
        """The `atac sort` kernels' limits (module-level atac_sort_limits)."""
        return atac_sort_limits()

    @staticmethod
    def atac_sort_table_slot(barcode, n_corr):
        """Home slot and capacity of the `atac sort` correction table (module-level atac_sort_table_slot)."""
        return atac_sort_table_slot(barcode, n_corr)

    def atac_sort_rad(self, chunk_bytes, chunk_off, observed, corrected, ref_lengths, bc_bytes: int = 4, d_ptr: int = 0, n_bytes: int = 0):
        """afq_atac_sort_rad: the chunks of an uncollated scATAC RAD in (host bytes, or d_ptr/n_bytes for bytes already on the
        device) with the correction map (observed -> corrected) and the references' lengths; a dict out: the distinct
        (ref, start, frag_len, bc) rows in that order with their count, and "stats"."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        obs = np.ascontiguousarray(observed, dtype=np.uint64)
        cor = np.ascontiguousarray(corrected, dtype=np.uint64)
        rl = np.ascontiguousarray(ref_lengths, dtype=np.uint32)
        if len(obs) != len(cor):
            raise ValueError("observed and corrected must have one length")
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        o_n = C.c_uint64()
        o_ref, o_start, o_len, o_bc, o_cnt = u32p(), u32p(), C.POINTER(C.c_uint16)(), u64p(), u32p()
        st = _abi.AfqAtacSortStats()
        self._check(self.lib.afq_atac_sort_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), bc_bytes, on_dev, obs.ctypes.data_as(u64p),
                                               cor.ctypes.data_as(u64p), len(obs), rl.ctypes.data_as(u32p), len(rl), C.byref(o_n), C.byref(o_ref),
                                               C.byref(o_start), C.byref(o_len), C.byref(o_bc), C.byref(o_cnt), C.byref(st)))
        n = int(o_n.value)
        try:
            mk = lambda p_, dt: (np.ctypeslib.as_array(p_, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt))
            return {"ref": mk(o_ref, np.uint32), "start": mk(o_start, np.uint32), "frag_len": mk(o_len, np.uint16), "bc": mk(o_bc, np.uint64),
                    "count": mk(o_cnt, np.uint32), "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_ref, o_start, o_len, o_bc, o_cnt):
                self.lib.afq_free(q)

    def gpl_hist_rad(self, chunk_bytes, chunk_off, bc_bytes: int = 4, umi_bytes: int = 4, expected_ori="both", d_ptr: int = 0, n_bytes: int = 0):
        """afq_gpl_hist_rad: the chunks of an uncollated RNA RAD in (host bytes, or d_ptr/n_bytes for bytes already on the device);
        a dict out: "bc" (the distinct barcodes of the records compatible with expected_ori - "both" / "either", "fw", "rc" - ascending),
        "count" (u64) and "stats" (n_records, n_compatible, max_ambig, n_long_records).  Position bytes: set_aln_extra_bytes."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        ori = _abi.GPL_ORI[expected_ori.lower()] if isinstance(expected_ori, str) else int(expected_ori)
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p = C.POINTER(C.c_uint64)
        o_n, o_bc, o_cnt, st = C.c_uint64(), u64p(), u64p(), _abi.AfqGplHistStats()
        self._check(self.lib.afq_gpl_hist_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), bc_bytes, umi_bytes, ori, on_dev, C.byref(o_n),
                                              C.byref(o_bc), C.byref(o_cnt), C.byref(st)))
        n = int(o_n.value)
        try:
            mk = lambda p_: (np.ctypeslib.as_array(p_, shape=(n,)).astype(np.uint64, copy=True) if n else np.zeros(0, np.uint64))
            return {"bc": mk(o_bc), "count": mk(o_cnt), "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_bc, o_cnt):
                self.lib.afq_free(q)

    def gpl_correct(self, observed, observed_count, retained, retained_count, barcode_len: int, neighborhood="substitution-or-shift-1",
                    resolution="unique", confidence=(39, 40), pseudocount: int = 1):
        """afq_gpl_correct: the correction decision of every observed barcode against the retained ones (both ascending, distinct);
        a dict out: "decision" (u8: _abi.GPL_EXACT ...), "target" (u32 index into retained, GPL_NO_TARGET without one),
        "target_count" (u64 per retained barcode) and "stats" (the eight CorrectionStats counters)."""
        obs = np.ascontiguousarray(observed, dtype=np.uint64)
        oc = np.ascontiguousarray(observed_count, dtype=np.uint64)
        ret = np.ascontiguousarray(retained, dtype=np.uint64)
        rc_ = np.ascontiguousarray(retained_count, dtype=np.uint64)
        if len(obs) != len(oc) or len(ret) != len(rc_):
            raise ValueError("a barcode list and its counts must have one length")
        nbh = _abi.GPL_NEIGHBORHOODS[neighborhood] if isinstance(neighborhood, str) else int(neighborhood)
        res = _abi.GPL_RESOLUTIONS[resolution] if isinstance(resolution, str) else int(resolution)
        u64p = C.POINTER(C.c_uint64)
        o_dec, o_tgt, o_tc, st = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint32)(), u64p(), _abi.AfqGplCorrectionStats()
        self._check(self.lib.afq_gpl_correct(self._h, obs.ctypes.data_as(u64p), oc.ctypes.data_as(u64p), len(obs), ret.ctypes.data_as(u64p),
                                             rc_.ctypes.data_as(u64p), len(ret), int(barcode_len), nbh, res, int(confidence[0]), int(confidence[1]),
                                             int(pseudocount), C.byref(o_dec), C.byref(o_tgt), C.byref(o_tc), C.byref(st)))
        try:
            mk = lambda p_, n, dt: (np.ctypeslib.as_array(p_, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt))
            return {"decision": mk(o_dec, len(obs), np.uint8), "target": mk(o_tgt, len(obs), np.uint32), "target_count": mk(o_tc, len(ret), np.uint64),
                    "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_dec, o_tgt, o_tc):
                self.lib.afq_free(q)

    @staticmethod
    def gpl_limits():
        """The generate-permit-list parse's limits (module-level gpl_limits)."""
        return gpl_limits()

    def gpl_multi_hist_rad(self, chunk_bytes, chunk_off, sample_observed, b0_bytes: int = 2, b1_bytes: int = 4, umi_bytes: int = 4, expected_ori="both",
                           d_ptr: int = 0, n_bytes: int = 0):
        """afq_gpl_multi_hist_rad: the chunks of an uncollated two-barcode RNA RAD in (host bytes, or d_ptr/n_bytes for bytes already on
        the device) and the routing entries (packed sample barcodes, ascending, distinct); a dict out: "entry" (u32 index into
        sample_observed), "cell" (u64) and "count" (u64) of the distinct pairs of the compatible, routed records, ascending by (entry,
        cell), and "stats" (n_records, n_compatible, n_routed, n_unrouted, n_long_records).  Position bytes: set_aln_extra_bytes."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        ent = np.ascontiguousarray(sample_observed, dtype=np.uint64)
        ori = _abi.GPL_ORI[expected_ori.lower()] if isinstance(expected_ori, str) else int(expected_ori)
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p = C.POINTER(C.c_uint64)
        o_n, o_ent, o_cell, o_cnt, st = C.c_uint64(), C.POINTER(C.c_uint32)(), u64p(), u64p(), _abi.AfqGplMultiHistStats()
        self._check(self.lib.afq_gpl_multi_hist_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), int(b0_bytes), int(b1_bytes), int(umi_bytes), ori, on_dev,
                                                    ent.ctypes.data_as(u64p), len(ent), C.byref(o_n), C.byref(o_ent), C.byref(o_cell), C.byref(o_cnt), C.byref(st)))
        n = int(o_n.value)
        try:
            mk = lambda p_, dt: (np.ctypeslib.as_array(p_, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt))
            return {"entry": mk(o_ent, np.uint32), "cell": mk(o_cell, np.uint64), "count": mk(o_cnt, np.uint64),
                    "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_ent, o_cell, o_cnt):
                self.lib.afq_free(q)

    @staticmethod
    def gpl_multi_limits():
        """The multi-barcode generate-permit-list parse's limits (module-level gpl_multi_limits)."""
        return gpl_multi_limits()

    def atac_gpl_hist_rad(self, chunk_bytes, chunk_off, bin_base, bc_bytes: int = 4, bin_size: int = 100000, d_ptr: int = 0, n_bytes: int = 0):
        """afq_atac_gpl_hist_rad: the chunks of an uncollated scATAC RAD in (host bytes, or d_ptr/n_bytes for bytes already on the device)
        and bin_base[ref_count + 1] (the first bin of every reference, ascending from 0); (bc, count, bins, stats dict) out: the distinct
        barcodes of ALL records ascending, their u64 counts, the u64 position bins of the records with one alignment, and the tallies."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        bb = np.ascontiguousarray(bin_base, dtype=np.uint64)
        if len(bb) < 1:
            raise ValueError("bin_base holds ref_count + 1 entries")
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p = C.POINTER(C.c_uint64)
        o_n, o_bc, o_cnt, o_bins, st = C.c_uint64(), u64p(), u64p(), u64p(), _abi.AfqAtacGplHistStats()
        self._check(self.lib.afq_atac_gpl_hist_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), bc_bytes, on_dev, bb.ctypes.data_as(u64p), len(bb) - 1,
                                                   int(bin_size), C.byref(o_n), C.byref(o_bc), C.byref(o_cnt), C.byref(o_bins), C.byref(st)))
        n, nbins = int(o_n.value), int(bb[-1])
        try:
            mk = lambda p_, k: (np.ctypeslib.as_array(p_, shape=(k,)).astype(np.uint64, copy=True) if k else np.zeros(0, np.uint64))
            return mk(o_bc, n), mk(o_cnt, n), mk(o_bins, nbins), {k: int(getattr(st, k)) for k, _ in st._fields_}
        finally:
            for q in (o_bc, o_cnt, o_bins):
                self.lib.afq_free(q)

    @staticmethod
    def atac_gpl_limits():
        """The `atac generate-permit-list` record pass's limits (module-level atac_gpl_limits)."""
        return atac_gpl_limits()

    def collate_rad(self, chunk_bytes, chunk_off, observed, corrected, cells, bc_bytes: int = 4, umi_bytes: int = 4, expected_ori="both", d_ptr: int = 0,
                    n_bytes: int = 0):
        """afq_collate_rad: the chunks of an uncollated RNA RAD in (host bytes, or d_ptr/n_bytes for bytes already on the device), the
        correction map observed -> corrected and the output cells in output order; a dict out: "bytes" (u8: one chunk per cell, back to
        back, headers included), "chunk_off" (u64, n_cells + 1), "nrec" (u32 per cell) and "stats".  Position bytes: set_aln_extra_bytes."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        obs = np.ascontiguousarray(observed, dtype=np.uint64)
        cor = np.ascontiguousarray(corrected, dtype=np.uint64)
        cel = np.ascontiguousarray(cells, dtype=np.uint64)
        if len(obs) != len(cor):
            raise ValueError("observed and corrected must have one length")
        ori = _abi.GPL_ORI[expected_ori.lower()] if isinstance(expected_ori, str) else int(expected_ori)
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p = C.POINTER(C.c_uint64)
        o_b, o_n, o_off, o_nrec, st = C.POINTER(C.c_uint8)(), C.c_uint64(), u64p(), C.POINTER(C.c_uint32)(), _abi.AfqCollateStats()
        self._check(self.lib.afq_collate_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), bc_bytes, umi_bytes, ori, on_dev, obs.ctypes.data_as(u64p),
                                             cor.ctypes.data_as(u64p), len(obs), cel.ctypes.data_as(u64p), len(cel), C.byref(o_b), C.byref(o_n), C.byref(o_off),
                                             C.byref(o_nrec), C.byref(st)))
        n, nc = int(o_n.value), len(cel)
        try:
            mk = lambda p_, k, dt: (np.ctypeslib.as_array(p_, shape=(k,)).astype(dt, copy=True) if k else np.zeros(0, dt))
            return {"bytes": mk(o_b, n, np.uint8), "chunk_off": mk(o_off, nc + 1, np.uint64), "nrec": mk(o_nrec, nc, np.uint32),
                    "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_b, o_off, o_nrec):
                self.lib.afq_free(q)

    @staticmethod
    def collate_limits():
        """The collate walks' and radix passes' limits (module-level collate_limits)."""
        return collate_limits()

    def convert_bam_rad(self, stream, span_off, n_ref: int, bc_bytes: int = 4, umi_bytes: int = 4, filter_best: bool = False, d_ptr: int = 0, n_bytes: int = 0):
        """afq_convert_bam_rad: the inflated record stream of a BAM in (host bytes, or d_ptr/n_bytes for bytes already on the device) with
        the table of record starts that cuts it into spans; a dict out: "bytes" (u8: the RAD chunks back to back, headers included),
        "chunk_off" (u64, n_chunks + 1), "nrec" (u32 per chunk) and "stats"."""
        off = np.ascontiguousarray(span_off, dtype=np.uint64)
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p = C.POINTER(C.c_uint64)
        o_b, o_n, o_off, o_nrec, o_nc, st = C.POINTER(C.c_uint8)(), C.c_uint64(), u64p(), C.POINTER(C.c_uint32)(), C.c_uint64(), _abi.AfqConvertStats()
        self._check(self.lib.afq_convert_bam_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), int(n_ref), bc_bytes, umi_bytes, int(bool(filter_best)), on_dev,
                                                 C.byref(o_b), C.byref(o_n), C.byref(o_off), C.byref(o_nrec), C.byref(o_nc), C.byref(st)))
        n, nc = int(o_n.value), int(o_nc.value)
        try:
            mk = lambda p_, k, dt: (np.ctypeslib.as_array(p_, shape=(k,)).astype(dt, copy=True) if k else np.zeros(0, dt))
            return {"bytes": mk(o_b, n, np.uint8), "chunk_off": mk(o_off, nc + 1, np.uint64), "nrec": mk(o_nrec, nc, np.uint32),
                    "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_b, o_off, o_nrec):
                self.lib.afq_free(q)

    @staticmethod
    def convert_limits():
        """The convert walks' and scans' limits (module-level convert_limits)."""
        return convert_limits()

    def collate_multi_rad(self, chunk_bytes, chunk_off, sample_observed, sample_index, corr_sample, corr_observed, corr_corrected, cell_sample, cell_bc,
                          sample_b0_out, b0_bytes: int = 2, b1_bytes: int = 4, umi_bytes: int = 4, expected_ori="both", d_ptr: int = 0, n_bytes: int = 0):
        """afq_collate_multi_rad: the chunks of an uncollated two-barcode RNA RAD in (host bytes, or d_ptr/n_bytes for bytes already on the
        device); the sample table sample_observed -> sample_index, the cell table (corr_sample, corr_observed) -> corr_corrected, the cells
        (cell_sample, cell_bc) in output order and sample_b0_out, the value written into b0 per sample.  The dict of collate_rad out."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
        u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)
        so, si, cs, co, cc, ls, lb, b0o = u64(sample_observed), u32(sample_index), u32(corr_sample), u64(corr_observed), u64(corr_corrected), u32(cell_sample), u64(cell_bc), u32(sample_b0_out)
        if len(so) != len(si) or not (len(cs) == len(co) == len(cc)) or len(ls) != len(lb):
            raise ValueError("the columns of a table must have one length")
        ori = _abi.GPL_ORI[expected_ori.lower()] if isinstance(expected_ori, str) else int(expected_ori)
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        o_b, o_n, o_off, o_nrec, st = C.POINTER(C.c_uint8)(), C.c_uint64(), u64p(), u32p(), _abi.AfqCollateMultiStats()
        self._check(self.lib.afq_collate_multi_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), int(b0_bytes), int(b1_bytes), int(umi_bytes), ori, on_dev,
                                                   so.ctypes.data_as(u64p), si.ctypes.data_as(u32p), len(so), cs.ctypes.data_as(u32p), co.ctypes.data_as(u64p),
                                                   cc.ctypes.data_as(u64p), len(cs), ls.ctypes.data_as(u32p), lb.ctypes.data_as(u64p), len(ls),
                                                   b0o.ctypes.data_as(u32p), len(b0o), C.byref(o_b), C.byref(o_n), C.byref(o_off), C.byref(o_nrec), C.byref(st)))
        n, nc = int(o_n.value), len(ls)
        try:
            mk = lambda p_, k, dt: (np.ctypeslib.as_array(p_, shape=(k,)).astype(dt, copy=True) if k else np.zeros(0, dt))
            return {"bytes": mk(o_b, n, np.uint8), "chunk_off": mk(o_off, nc + 1, np.uint64), "nrec": mk(o_nrec, nc, np.uint32),
                    "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_b, o_off, o_nrec):
                self.lib.afq_free(q)

    @staticmethod
    def collate_multi_limits():
        """Multi-barcode collate's limits (module-level collate_multi_limits)."""
        return collate_multi_limits()

    def atac_collate_rad(self, chunk_bytes, chunk_off, observed, corrected, cells, bc_bytes: int = 4, d_ptr: int = 0, n_bytes: int = 0):
        """afq_atac_collate_rad: the chunks of an uncollated scATAC RAD in (host bytes, or d_ptr/n_bytes for bytes already on the device),
        the correction map observed -> corrected and the cells in output order; a dict out: "bytes" (u8: one chunk per cell that kept a
        record, back to back, headers included), "chunk_off" (u64, n_out + 1), "nrec" (u32 per chunk), "cell" (u32 per chunk: the index
        into `cells`) and "stats"."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        obs = np.ascontiguousarray(observed, dtype=np.uint64)
        cor = np.ascontiguousarray(corrected, dtype=np.uint64)
        cel = np.ascontiguousarray(cells, dtype=np.uint64)
        if len(obs) != len(cor):
            raise ValueError("observed and corrected must have one length")
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        o_b, o_n, o_nc, o_off, o_nrec, o_cell, st = C.POINTER(C.c_uint8)(), C.c_uint64(), C.c_uint64(), u64p(), u32p(), u32p(), _abi.AfqAtacCollateStats()
        self._check(self.lib.afq_atac_collate_rad(self._h, ptr, nb, off.ctypes.data_as(u64p), len(off), bc_bytes, on_dev, obs.ctypes.data_as(u64p),
                                                  cor.ctypes.data_as(u64p), len(obs), cel.ctypes.data_as(u64p), len(cel), C.byref(o_b), C.byref(o_n),
                                                  C.byref(o_nc), C.byref(o_off), C.byref(o_nrec), C.byref(o_cell), C.byref(st)))
        n, nc = int(o_n.value), int(o_nc.value)
        try:
            mk = lambda p_, k, dt: (np.ctypeslib.as_array(p_, shape=(k,)).astype(dt, copy=True) if k else np.zeros(0, dt))
            return {"bytes": mk(o_b, n, np.uint8), "chunk_off": mk(o_off, nc + 1, np.uint64), "nrec": mk(o_nrec, nc, np.uint32),
                    "cell": mk(o_cell, nc, np.uint32), "stats": {k: int(getattr(st, k)) for k, _ in st._fields_}}
        finally:
            for q in (o_b, o_off, o_nrec, o_cell):
                self.lib.afq_free(q)

    @staticmethod
    def atac_collate_limits():
        """The `atac collate` walks' and radix passes' limits (module-level atac_collate_limits)."""
        return atac_collate_limits()

    def atac_dedup_rad(self, chunk_bytes, chunk_off, bc_bytes: int = 4, d_ptr: int = 0, n_bytes: int = 0, copy: bool = True):
        """afq_atac_dedup_rad: collated scATAC chunks in (host bytes, or d_ptr/n_bytes for bytes already on the device),
        (cell_ptr, bc, ref, start, frag_len, count, stats dict) out."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        n_cells = len(off)
        if d_ptr:
            ptr, nb, on_dev = C.c_void_p(d_ptr), n_bytes, 1
        else:
            b = np.ascontiguousarray(np.frombuffer(chunk_bytes, dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) else chunk_bytes)
            ptr, nb, on_dev = b.ctypes.data_as(C.c_void_p), b.nbytes, 0
        o_ptr, o_bc, o_ref, o_start = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        o_len, o_cnt = C.POINTER(C.c_uint16)(), C.POINTER(C.c_uint16)()
        st = _abi.AfqAtacStats()
        self._check(self.lib.afq_atac_dedup_rad(self._h, ptr, nb, off.ctypes.data_as(C.POINTER(C.c_uint64)), n_cells, bc_bytes, on_dev,
                                                C.byref(o_ptr), C.byref(o_bc), C.byref(o_ref), C.byref(o_start), C.byref(o_len), C.byref(o_cnt), C.byref(st)))
        cp = np.ctypeslib.as_array(o_ptr, shape=(n_cells + 1,)).copy()
        n = int(cp[-1])
        stats = {k: int(getattr(st, k)) for k, _ in st._fields_}
        if not copy:   # views over the library's (pinned) arrays, handed back to it when the last view dies
            import weakref

            lib, ptrs = self.lib, (o_ptr, o_bc, o_ref, o_start, o_len, o_cnt)

            class _Own:
                pass

            own = _Own()
            weakref.finalize(own, lambda: [lib.afq_free(q) for q in ptrs])

            def view(p_, k):
                a = np.ctypeslib.as_array(p_, shape=(max(k, 1),))[:k]
                a.flags.writeable = False
                keep = np.ndarray.__new__(_Held, a.shape, a.dtype, a, 0, a.strides)
                keep._own = own
                return keep

            return cp, view(o_bc, n_cells), view(o_ref, n), view(o_start, n), view(o_len, n), view(o_cnt, n), stats
        try:
            mk = lambda p_, dt, k: (np.ctypeslib.as_array(p_, shape=(k,)).astype(dt, copy=True) if k else np.zeros(0, dt))
            return cp, mk(o_bc, np.uint64, n_cells), mk(o_ref, np.uint32, n), mk(o_start, np.uint32, n), mk(o_len, np.uint16, n), mk(o_cnt, np.uint16, n), stats
        finally:
            for q in (o_ptr, o_bc, o_ref, o_start, o_len, o_cnt):
                self.lib.afq_free(q)
