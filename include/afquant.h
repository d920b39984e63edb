/*
 * afquant.h — C ABI of the MI355X-native `alevin-fry quant` hot path.
 *
 * The reference (COMBINE-lab/alevin-fry v0.18.0, pure Rust) has no FFI layer:
 * the hot path is the body of the per-cell loop in `run_worker_thread`
 * (src/quant.rs:733-1322), configured by `WorkerConfig` (src/quant.rs:398-416).
 * This header is the seam a Rust host would bind instead of that loop body:
 * "collated chunk bytes in -> sparse row + flags out".  Every entry point
 * cites the reference item it replaces.  Plain pointers and sizes only.
 *
 * All functions return 0 on success or a negative AFQ_ERR_* code; the text of
 * the last error on a context is available from afq_last_error().  Nothing in
 * this library aborts the process (the reference panics / exit(1)s instead:
 * src/pugutils.rs:1148-1151, Cargo.toml:100-108).
 */
#ifndef AFQUANT_H
#define AFQUANT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFQ_ABI_VERSION 3   /* 3: afq_result.mmrate and afq_snappy_decode_device are gone, afq_em_resize_count and afq_mono_cell_count are new */

/* error codes */
#define AFQ_OK 0
#define AFQ_ERR_INVALID_ARG (-1)  /* null pointer, bad enum, inconsistent sizes  */
#define AFQ_ERR_BAD_INPUT (-2)    /* malformed chunk bytes / ref id out of range */
#define AFQ_ERR_UNSUPPORTED (-3)  /* valid request the device path cannot take   */
/* What AFQ_ERR_UNSUPPORTED stands for today (the reference has none of these limits, quant.rs:733-757; never approximated, the
 * whole batch is refused and afq_last_error names the cell):
 *   - UMIs over 22 nt, gene-id spaces over 2^20, more than two barcode levels;
 *   - parsimony: a cell of 2^22 reads or more; a cell of 2^20 .. 2^22 reads goes through the partition-parallel kernels and is
 *     fine as long as they can finish it - whatever its graph looks like under the default --large-graph-thresh: components of
 *     any size, pair lists of any length.  Only when they have to hand it to the one-workgroup kernel (a UMI partition over 256
 *     reads: UMIs that share their low bases, e.g. a constant primer tail; gene-level labels or an 8-byte UMI field send every
 *     cell there) that kernel's 2^20-read limit applies;
 *   - parsimony: a component over 4096 vertices under a --large-graph-thresh raised beyond that;
 *   - multi-barcode records (bc_split) that carry alignment positions (afq_set_aln_extra_bytes). */
#define AFQ_ERR_HIP (-4)          /* a HIP runtime call failed                   */
#define AFQ_ERR_NO_DEVICE (-5)    /* no usable gfx950 device                     */
#define AFQ_ERR_STATE (-6)        /* call sequence error (collect before submit) */
#define AFQ_ERR_OOM (-7)

/* ResolutionStrategy, src/quant.rs:82-114 (CLI spellings in the comments). */
typedef enum afq_resolution {
    AFQ_RES_TRIVIAL = 0,           /* trivial            */
    AFQ_RES_CR_LIKE = 1,           /* cr-like            */
    AFQ_RES_CR_LIKE_EM = 2,        /* cr-like-em         */
    AFQ_RES_PARSIMONY_EM = 3,      /* parsimony-em       */
    AFQ_RES_PARSIMONY = 4,         /* parsimony          */
    AFQ_RES_PARSIMONY_GENE_EM = 5, /* parsimony-gene-em  */
    AFQ_RES_PARSIMONY_GENE = 6     /* parsimony-gene     */
} afq_resolution;

/* SplicedAmbiguityModel (src/quant.rs, `--sa-model`). */
typedef enum afq_sa_model { AFQ_SA_WINNER_TAKE_ALL = 0, AFQ_SA_PREFER_AMBIG = 1 } afq_sa_model;

/* per-cell flag bits in afq_result.flags */
#define AFQ_CELL_TINY_PATH 0x1u /* used_fast_path,   src/quant.rs:794-797      */
#define AFQ_CELL_ALT_RES 0x2u   /* alt_resolution,   src/quant.rs:966, 1131     */
#define AFQ_CELL_EMPTY 0x4u     /* num_expr == 0,    src/quant.rs:1173          */

/*
 * Mirror of WorkerConfig (src/quant.rs:398-416) — the part of QuantOpts
 * (src/prog_opts.rs:24-44) that reaches the per-cell code — plus the record
 * field widths the reference gets from the RAD prelude (src/convert.rs:323-344).
 * POD; copied by afq_create.
 */
typedef struct afq_config {
    uint32_t abi_version;        /* AFQ_ABI_VERSION                                              */
    uint32_t resolution;         /* afq_resolution                                               */
    uint32_t sa_model;           /* afq_sa_model (forced to WTA when !usa_mode, quant.rs:1456)   */
    uint32_t usa_mode;           /* 3-column tg-map: spliced gid even, unspliced odd             */
    uint32_t num_genes;          /* gene-id space of tid_to_gid (USA: 2*G, spliced/unspliced)    */
    uint32_t num_rows;           /* output columns: num_genes, or 3*G in USA (quant.rs:1627-1645)*/
    uint32_t small_thresh;       /* tiny_cell_thresh; cells with nrec < this take the tiny path  */
    uint32_t large_graph_thresh; /* PUG component size above which cr-like is used (pugutils.rs:1055) */
    uint32_t pug_exact_umi;      /* 1: only identical UMIs induce PUG edges (--umi-edit-dist 0)  */
    uint32_t em_init_uniform;    /* EmInitType::Uniform instead of Informative (em.rs:37-41)     */
    uint32_t bc_bytes;           /* width of the barcode field in a record: 1,2,4,8              */
    uint32_t umi_bytes;          /* width of the UMI field in a record: 1,2,4,8                  */
    uint32_t profile;            /* 1: bracket every kernel with HIP events (afq_get_kernel_times)*/
    uint32_t umi_len;            /* UMI length in bases when the caller knows it (the RAD file tag `ulen`); 0 = unknown.
                                    Only bounds the 1-mismatch neighbour probes of the PUG (positions past the UMI
                                    cannot differ), so a value that is too SMALL would lose edges: pass 0 when unsure. */
    uint32_t dump_eq;            /* -d / dump_eq (quant.rs:1282-1307): also keep each cell's gene-level equivalence classes,
                                    handed out by afq_result_eqclasses(); -em resolutions only                  */
    uint32_t bc_split;           /* multi-barcode records (10x Flex: b0 = sample index, b1 = cell barcode) whose two barcode
                                    integers differ in width: bc_bytes = w0 + w1 (2..8) and bc_split = w0 (1..4, w1 = bc_bytes - w0
                                    in 1..4).  The batch is rewritten on the device with both as 4-byte fields and the reported
                                    barcode is b0 | b1 << 32.  0 = the barcode is one field of 1, 2, 4 or 8 bytes (equal-width
                                    pairs travel that way too: b0 | b1 << 8 w0).                                               */
    /* -b / --num-bootstraps with --summary-stat (src/quant.rs:1028-1038, em.rs:585-757; -em resolutions only, main.rs:713-724):
       per non-tiny cell, num_bootstraps times: the counts of its gene-level classes are redrawn from a multinomial over the
       observed counts and re-estimated by the EM from a random start; afq_result_bootstraps() hands out the per-column mean
       and variance.  The reference draws from an unseeded thread RNG - its numbers are not reproducible; here the draws
       are Philox4x32-10 keyed by boot_seed and the cell's index (first_cell_index + i), so a run is reproducible and does
       not depend on batching. */
    uint32_t num_bootstraps;
    uint32_t summary_stat;       /* 1: mean and E[x^2]-mean^2 (em.rs:673-683); 0: mean and the n-1 sample variance over the
                                    replicates (quant.rs:185-210).  Either way only the two summaries are produced, as in the reference */
    uint64_t boot_seed;
} afq_config;

typedef struct afq_ctx afq_ctx;

/*
 * One result batch = what run_worker_thread accumulates for a run of cells:
 * `expressed_ind/expressed_vec` per cell (src/quant.rs:1156-1168, 808-845) as
 * CSR, plus the per-cell scalars it logs.  Library-owned until
 * afq_result_release(); all pointers are host memory.
 */
typedef struct afq_result {
    uint64_t n_cells;
    uint64_t first_cell_index; /* cell_num of cell 0 (MetaChunk.first_chunk_index, quant.rs:734) */
    uint64_t nnz;
    const uint64_t* cell_ptr; /* [n_cells+1] offsets into gene/val                               */
    const uint32_t* gene;     /* [nnz] output column, ascending within a cell                     */
    const float* val;         /* [nnz] count > 0                                                  */
    const uint64_t* bc;       /* [n_cells] collate_key of the cell's first record (quant.rs:757)  */
    const uint32_t* nrec;     /* [n_cells] records in the chunk                                   */
    const uint8_t* flags;     /* [n_cells] AFQ_CELL_*                                             */
    /* (`trivial` also computes a multi-mapping rate in the reference, pugutils.rs:909 - stored at quant.rs:936 and never read
       or written anywhere: it is not part of the result) */
    void* opaque;
} afq_result;

/*
 * Replaces the worker set-up of do_quantify (src/quant.rs:1678-1765): builds a
 * per-device context holding the config and the transcript->gene table
 * (`tid_to_gid`, src/utils.rs:487-662; len = ref_count).  `device` is the HIP
 * device ordinal.  One context per device; contexts are independent.
 */
int afq_create(const afq_config* cfg, const uint32_t* tid_to_gid, uint32_t ref_count, int device,
               afq_ctx** out);
void afq_destroy(afq_ctx* ctx);

/*
 * Replaces handing a MetaChunk of cells to a worker (src/quant.rs:733-757).
 * `bytes` are collated-RAD chunks exactly as on disk, back to back or not:
 * chunk i starts at bytes[chunk_off[i]] with its 8-byte header
 * (nbytes:u32 incl. header, nrec:u32; src/convert.rs:473-481) followed by nrec
 * records `na:u32, bc, umi, na x u32(ori<<31|ref)` (src/convert.rs:124-144).
 * One chunk = one cell.  The caller keeps ownership; the bytes are copied to
 * the device before return.  Results are produced asynchronously on the
 * context's stream; afq_collect waits for them.
 */
int afq_submit(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off,
               uint32_t n_cells, uint64_t first_cell_index);

/*
 * Same, for a host that would rather be asked for the bytes than hold them all in memory (the reference's producer reads
 * the collated file chunk by chunk, src/quant.rs:1773-1784): `read(user, offset, dst, len)` fills dst with bytes
 * [offset, offset + len) of the chunk stream and returns 0; it is called from several threads at once, with dst in pinned
 * staging memory, while earlier parts are already on their way to the device (a pread on a file descriptor is all it has
 * to be).  chunk_hdr = the 8-byte chunk headers (nbytes, nrec per cell), which the host has from walking the chunk table.
 */
typedef int (*afq_read_fn)(void* user, uint64_t offset, void* dst, size_t len);
int afq_submit_reader(afq_ctx* ctx, afq_read_fn read, void* user, size_t n_bytes, const uint64_t* chunk_off,
                      const uint32_t* chunk_hdr, uint32_t n_cells, uint64_t first_cell_index);

/*
 * Same, for chunk bytes already resident in this context's device memory
 * (what a host that overlaps H2D itself would use; bench.py times this form).
 * `d_bytes` must stay valid until afq_collect returns.  `chunk_off` is host
 * memory.
 */
int afq_submit_device(afq_ctx* ctx, const void* d_bytes, size_t n_bytes, const uint64_t* chunk_off,
                      uint32_t n_cells, uint64_t first_cell_index);

/*
 * Records that carry a position per alignment (KnownRecordType::RnaShortPos, src/utils.rs:313-377: alignment tags
 * compressed_ori_refid:u32 then pos of `e` bytes).  A record is then `na:u32, bc, umi, na x {u32(ori<<31|ref), pos}` and the
 * reference quantifies it exactly as a plain record (src/quant.rs:1977-1990, BasicEqClassPayload): positions never reach a
 * count.  The batch is rewritten on the device without them before the decode.  e = 1, 2, 4 or 8; 0 = plain records (the
 * default).  Applies to every later submit of the context (all three forms) until changed.  Returns AFQ_ERR_INVALID_ARG for
 * any other width, AFQ_ERR_UNSUPPORTED for a nonzero e on a context whose config has bc_split set (multi-barcode records with
 * positions), AFQ_ERR_STATE while a batch is pending.
 */
int afq_set_aln_extra_bytes(afq_ctx* ctx, uint32_t e);

/* Waits for the submitted batch and returns its rows (src/quant.rs:1131-1179, 1266-1268). */
int afq_collect(afq_ctx* ctx, afq_result* out);
void afq_result_release(afq_result* res);

/*
 * cfg.dump_eq: what the reference copies out of `gene_eqc` per cell for -d (src/quant.rs:1282-1307) - the gene-level
 * equivalence classes left by the resolution, label = ascending gene ids of tid_to_gid's id space (USA: spliced 2k,
 * unspliced 2k+1), count = molecules.  Cells that took the tiny-cell path have none (they never touch gene_eqc).
 * The reference walks a hash map, so the order of a cell's classes is not defined there; here: single-gene (and USA
 * S+U of one gene) labels by output column, then the others in lexicographic order.  Owned by `res`.
 */
typedef struct afq_eqclasses {
    uint64_t n_cells, n_classes, n_words;
    const uint64_t* cell_ptr;  /* [n_cells+1]   classes of cell i: cell_ptr[i] .. cell_ptr[i+1]     */
    const uint64_t* label_ptr; /* [n_classes+1] label of class k: labels[label_ptr[k] .. label_ptr[k+1]) */
    const uint32_t* labels;    /* [n_words]                                                       */
    const uint32_t* count;     /* [n_classes]                                                     */
} afq_eqclasses;
int afq_result_eqclasses(const afq_result* res, afq_eqclasses* out);

/*
 * cfg.num_bootstraps > 0: what BootstrapHelper::record_cell[_from_replicates] collects (src/quant.rs:157-210): per cell
 * the non-zero bootstrap means and variances, as two CSR matrices over the same cells.  Columns are the alpha indices the
 * reference's run_bootstrap uses - the gene ids of gene_eqc's labels (in USA mode that is the spliced/unspliced id 2k /
 * 2k+1, NOT the S/U/A output column: run_bootstrap_with_scratch is handed gene_eqc as is, quant.rs:1028-1038).
 * Tiny-path cells have no bootstraps.  Owned by `res`.
 */
typedef struct afq_bootstraps {
    uint64_t n_cells;
    const uint64_t* mean_ptr; const uint32_t* mean_col; const float* mean_val;   /* [n_cells+1], [nnz], [nnz] */
    const uint64_t* var_ptr;  const uint32_t* var_col;  const float* var_val;
} afq_bootstraps;
int afq_result_bootstraps(const afq_result* res, afq_bootstraps* out);

/*
 * The per-cell work of `alevin-fry infer` (src/infer.rs:31-426): one EM (em_optimize_subset, EmInitType::Informative,
 * USA offsets (num_alphas/3, 2*num_alphas/3) when usa_mode) per row of an equivalence-class count matrix.
 *   eq_labels / eq_label_ptr : the global classes (IndexedEqList::init_from_eqc_file): class e = eq_labels[eq_label_ptr[e] ..
 *                              eq_label_ptr[e+1]), output columns (a gene_eqclass.txt.gz as `quant -d` writes it)
 *   cell_ptr / cell_eq / cell_count : the count matrix in CSR, class ids ascending within a row (what sprs' to_csr() gives),
 *                              counts already rounded to integers (infer.rs:389)
 * `out` gets the non-zero abundances per cell (gene/val ascending by column; bc, nrec, flags are 0).  The context's own
 * resolution settings play no part.  Release with afq_result_release().
 */
int afq_infer(afq_ctx* ctx, const uint32_t* eq_labels, const uint64_t* eq_label_ptr, uint32_t n_eq, const uint64_t* cell_ptr,
              const uint32_t* cell_eq, const uint32_t* cell_count, uint32_t n_cells, uint32_t num_alphas, uint32_t usa_mode,
              afq_result* out);

/*
 * Per-cell fragment de-duplication of `alevin-fry atac deduplicate`
 * (src/atac/deduplicate.rs:199-237, HitInfo order src/atac/sort.rs:37-64).
 * Input per cell: the (ref, start, frag_len) of every record that has exactly
 * one alignment of map_type 4; output: distinct fragments in
 * (ref,start,frag_len) order with their multiplicity (u16, as in the reference).
 * `cell_ptr` has n_cells+1 entries.  Output arrays are malloc'd; free with
 * afq_free().
 */
int afq_atac_dedup(afq_ctx* ctx, const uint32_t* ref, const uint32_t* start,
                   const uint16_t* frag_len, const uint64_t* cell_ptr, uint32_t n_cells,
                   uint64_t** out_cell_ptr, uint32_t** out_ref, uint32_t** out_start,
                   uint16_t** out_frag_len, uint16_t** out_count);
void afq_free(void* p);

/*
 * The same, from the collated-RAD chunks themselves: the record loop of deduplicate.rs:199-218 (walk the
 * AtacSeqReadRecords `na:u32, bc, na x {ref:u32, type:u8, start_pos:u32, frag_len:u16}` - tests/atac_integration.rs:110-121 -
 * keep those with exactly one alignment of map_type 4, count the rest) runs on the device in front of the sort.
 * `bytes` / `chunk_off` as for afq_submit (bytes_on_device != 0: `bytes` is device memory of this context's device).
 * Outputs as afq_atac_dedup, plus the barcode of every cell; free each with afq_free().
 */
typedef struct afq_atac_stats {
    uint64_t n_records;          /* records read                                                                  */
    uint64_t n_multimapped;      /* "records with greater than 1 mapping", deduplicate.rs:210-212                 */
    uint64_t n_not_mapped_pair;  /* neither kept nor multi-mapped (no alignment, or one that is not type 4), :213-215 */
    uint64_t n_distinct;         /* distinct fragments over all cells                                             */
    uint64_t n_deduplicated;     /* distinct fragments seen more than once (the run length before `as u16`), :224 */
    uint64_t n_long_fragments;   /* distinct fragments with frag_len >= 2000 (left out of the BED, :47-63)        */
    uint64_t n_fallback_cells;   /* cells the walk-free parse could not prove and walked record by record         */
} afq_atac_stats;
int afq_atac_dedup_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_cells,
                       uint32_t bc_bytes, int bytes_on_device, uint64_t** out_cell_ptr, uint64_t** out_bc, uint32_t** out_ref,
                       uint32_t** out_start, uint16_t** out_frag_len, uint16_t** out_count, afq_atac_stats* stats);

/*
 * `alevin-fry atac sort` (src/atac/sort.rs) on the device: every record of an UNCOLLATED scATAC RAD - the mapper's chunks, whose
 * records carry a barcode each - is walked, a record is kept iff it has exactly one alignment (sort.rs:121-123; no map_type
 * filter, unlike deduplicate) and its barcode is one of `observed`, and the kept fragments come back as the distinct
 * (ref, start, frag_len, corrected barcode) tuples in that order (barcode as an integer, sort.rs:47-59) with their multiplicity
 * (u32: the reference counts in a usize, sort.rs:74).  Fragments of 2000 bases and more are INCLUDED (the cut at sort.rs:75
 * belongs to the writer) and counted in n_long_fragments.
 *   observed / corrected : the correction map, n_corrections pairs in any order; the same pair twice is fine, one observed
 *                          barcode with two corrected ones is AFQ_ERR_BAD_INPUT
 *   ref_lengths          : the prelude's ref_lengths tag; ref >= ref_count or start_pos >= ref_lengths[ref] in a record with one
 *                          alignment is AFQ_ERR_BAD_INPUT, as are records that do not tile their chunk or do not number its
 *                          nrec - the message names the chunk, nothing outside `bytes` is read, the context stays usable
 * Limits (AFQ_ERR_UNSUPPORTED): 2^32 records, 2^31 distinct corrected barcodes, 2^31 position bins, 2^30 map entries per call.
 * An input that does not fit the device with its staging is AFQ_ERR_OOM (sizes in the message); one call is one device fill.
 * `bytes` / `chunk_off` / bytes_on_device as for afq_atac_dedup_rad.  Free each output array with afq_free().
 */
typedef struct afq_atac_sort_stats {
    uint64_t n_records;             /* records read                                                        */
    uint64_t n_unmapped;            /* records without an alignment                                        */
    uint64_t n_multimapped;         /* records with more than one                                          */
    uint64_t n_uncorrected;         /* one alignment, barcode not in the map                               */
    uint64_t n_kept;                /* fragments sorted                                                    */
    uint64_t n_distinct;            /* rows returned                                                       */
    uint64_t n_long_fragments;      /* rows with frag_len >= 2000                                          */
    uint64_t n_repartitioned_bins;  /* position bins above the leaf cap, split again by their key bits     */
} afq_atac_sort_stats;
int afq_atac_sort_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks,
                      uint32_t bc_bytes, int bytes_on_device, const uint64_t* observed, const uint64_t* corrected,
                      uint64_t n_corrections, const uint32_t* ref_lengths, uint32_t ref_count, uint64_t* out_n, uint32_t** out_ref,
                      uint32_t** out_start, uint16_t** out_frag_len, uint64_t** out_bc, uint32_t** out_count,
                      afq_atac_sort_stats* stats);
/* out[0] = bin shift S (a position bin is 2^S bases), out[1] = leaf cap (keys one workgroup sorts in LDS), out[2] = a segment
 * with MORE keys than this is partitioned again, out[3] = bytes of a chunk the parse stages per trip.  For tests, which derive
 * their boundary shapes from these. */
void afq_atac_sort_limits(uint32_t out[4]);
/* out[0] = leaves of at most this many keys are sorted by the smaller workgroup, out[1] / out[2] = threads of the smaller / the
 * larger leaf workgroup (a leaf's run heads are compacted a slice of that many at a time), out[3] = bytes the parse stages
 * behind a tile (the head and one alignment of a record that starts on the tile's last byte).  For tests, as above. */
void afq_atac_sort_leaf_limits(uint32_t out[4]);
/* The correction table afq_atac_sort_rad builds for n_corrections entries: its capacity (the smallest power of two
 * >= max(2, 2 * n_corrections); open addressing, the next slot modulo the capacity on a collision) and the home slot of
 * `barcode` in it.  For tests, which build probe chains of a stated length from these.  Either pointer may be NULL. */
void afq_atac_sort_table_slot(uint64_t barcode, uint64_t n_corrections, uint32_t* home_slot, uint32_t* capacity);

/*
 * `generate-permit-list`, the device half: the barcode histogram of an UNCOLLATED single-barcode RNA RAD.
 *
 * `bytes` / `chunk_off` are the mapper's chunks as for afq_atac_sort_rad; a record is `na u32, barcode (bc_bytes), umi
 * (umi_bytes), na x (u32 ref | orientation bit 31, + the position bytes of afq_set_aln_extra_bytes)`.  A record counts if it
 * is compatible with expected_ori (cellfilter.rs:1698-1771 of the reference): 0 = both: always; 1 = fw: some alignment word
 * has bit 31 set; 2 = rc: some alignment word has bit 31 clear; a record with na == 0 counts only under `both`.
 *
 * Out: the distinct barcodes of the compatible records, ascending, with their u64 counts (malloc'd; afq_free), and `stats`.
 * One call is one fill of the device: a host with a file larger than the device calls once per part and merges the sorted
 * histograms, summing n_records / n_compatible and taking the largest max_ambig.
 * Errors: AFQ_ERR_BAD_INPUT "chunk <i>: ..." for a chunk outside the buffer, a record head or an alignment list that runs
 * past its chunk's end, records that do not tile nbytes or do not number nrec; AFQ_ERR_UNSUPPORTED for 2^30 records or more
 * in one call; AFQ_ERR_OOM (with the sizes) when input and tables do not fit the device.
 */
typedef struct afq_gpl_hist_stats {
    uint64_t n_records;      /* records of the chunks                                                            */
    uint64_t n_compatible;   /* ... compatible with expected_ori (= the sum of the counts)                       */
    uint64_t max_ambig;      /* the largest na among the COMPATIBLE records (`max-ambig-record`)                 */
    uint64_t n_long_records; /* records whose alignment words the whole wave tested out of global memory: more than
                                afq_gpl_limits()[2] alignments, under fw / rc                                       */
} afq_gpl_hist_stats;
int afq_gpl_hist_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes,
                     uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, uint64_t* out_n, uint64_t** out_bc, uint64_t** out_count,
                     afq_gpl_hist_stats* stats);
/*
 * `generate-permit-list`, the correction decisions (CorrectionIndex::resolve, barcode_correction.rs:427-474, 659-704, for
 * retained sources that are their own canonical target): for every observed barcode, against the retained barcodes with their
 * exact counts.  Both lists ascend without duplicates (else AFQ_ERR_INVALID_ARG); every barcode fits 2 * barcode_len bits
 * (else AFQ_ERR_BAD_INPUT); barcode_len is 1..32.  neighborhood: 0 = hamming-1, 1 = substitution-or-shift-1.  resolution:
 * 0 = unique (confidence and pseudocount are ignored), 1 = frequency: a candidate's weight is exact count + pseudocount
 * (pseudocount >= 1), the winner is the greatest (weight, target), accepted iff winner / total >= conf_num / conf_den exactly.
 * That test is winner * conf_den >= conf_num * total in 128 bits: both products of two u64 fit, and winner and total fit a u64
 * because every weight is kept below 2^55 (a larger exact count + pseudocount is AFQ_ERR_UNSUPPORTED) and an observed barcode
 * has at most 3 * 32 + 31 * 13 = 499 candidates.  So every conf_den != 0 with conf_num <= conf_den serves; others are
 * AFQ_ERR_INVALID_ARG.
 * Out (malloc'd; afq_free): decision[n_observed] (0 exact, 1 corrected, 2 ambiguous, 3 not found), target[n_observed] (index
 * into `retained`, 0xFFFFFFFF without one), target_count[n_retained] (the sum of the accepted observations' counts), `stats`.
 * The full theoretical neighbourhood of permit_map.bin is the same call with the neighbours as `observed` and counts of 0.
 */
typedef struct afq_gpl_correction_stats {
    uint64_t exact_distinct, exact_reads, corrected_distinct, corrected_reads, ambiguous_distinct, ambiguous_reads, not_found_distinct, not_found_reads;
} afq_gpl_correction_stats;
int afq_gpl_correct(afq_ctx* ctx, const uint64_t* observed, const uint64_t* observed_count, uint64_t n_observed, const uint64_t* retained,
                    const uint64_t* retained_count, uint64_t n_retained, uint32_t barcode_len, uint32_t neighborhood, uint32_t resolution,
                    uint64_t conf_num, uint64_t conf_den, uint64_t pseudocount, uint8_t** out_decision, uint32_t** out_target,
                    uint64_t** out_target_count, afq_gpl_correction_stats* stats);
/* out[0] = bytes of a chunk the GPL parse stages per trip, out[1] = bytes staged behind them (they hold the widest head and
 * out[2] of the widest alignments), out[2] = a record with more alignments than this is a long record, out[3] = 0.  For tests. */
void afq_gpl_limits(uint32_t out[4]);
/* The counting table afq_gpl_hist_rad builds for n_kept compatible records of bc_bytes-wide barcodes: its capacity (the smallest
 * power of two >= max(2, 2 * min(n_kept, 2^(8 bc_bytes))); open addressing, the next slot modulo the capacity on a collision)
 * and the home slot of `barcode` in it.  For tests.  Either pointer may be NULL. */
void afq_gpl_table_slot(uint64_t barcode, uint64_t n_kept, uint32_t bc_bytes, uint32_t* home_slot, uint32_t* capacity);

/*
 * Multi-barcode `generate-permit-list`, the device half (do_generate_permit_list_multi_bc, src/cellfilter.rs:789-1381 of the
 * reference): the (routing entry, cell barcode) histogram of an UNCOLLATED two-barcode RNA RAD.
 *
 * `bytes` / `chunk_off` / bytes_on_device / expected_ori and the compatibility rule are afq_gpl_hist_rad's; a record is `na u32,
 * b0 (b0_bytes), b1 (b1_bytes), umi (umi_bytes), na x (u32 ref | orientation bit 31, + the position bytes of
 * afq_set_aln_extra_bytes)`; b0_bytes and b1_bytes are 1, 2 or 4, umi_bytes 1, 2, 4 or 8.  sample_observed[n_entries] are the
 * routing entries: packed sample barcodes, ascending and distinct (else AFQ_ERR_INVALID_ARG), each fitting b0_bytes (else
 * AFQ_ERR_BAD_INPUT); n_entries == 0 is legal (every record is then unrouted), more than 2^31 is AFQ_ERR_UNSUPPORTED.
 *
 * Every compatible record looks its b0 up among the entries: a hit at index e counts the pair (e, b1), a miss adds to n_unrouted.
 * What an entry means - an exact source, a corrected neighbour, an alias, a barcode whose decision is deferred - is the host's.
 *
 * Out (malloc'd; afq_free): the distinct pairs, ascending by (entry, cell), with their u64 counts, and `stats`.  All counts are
 * integer sums and the host sorts: the output is a function of the input alone, run to run.  The entry table is afq_atac_sort_rad's
 * correction table, so afq_atac_sort_table_slot(b0, n_entries, ..) describes it; the counting table is afq_gpl_hist_rad's over the
 * keys entry << 32 | b1, so afq_gpl_table_slot(key, n_routed, 8, ..) describes it.  One call is one fill of the device: a host with
 * a larger file calls once per part with the same entries, merges the sorted outputs and sums the stats.
 * Errors: AFQ_ERR_BAD_INPUT "chunk <i>: ..." for a chunk outside the buffer, a head or an alignment list that runs past its chunk,
 * records that do not tile nbytes or do not number nrec (nothing outside `bytes` is read, no partial histogram is returned, the
 * context stays usable); AFQ_ERR_UNSUPPORTED for 2^30 records or more in one call; AFQ_ERR_OOM (with the sizes) when input and
 * tables do not fit the device.
 */
typedef struct afq_gpl_multi_hist_stats {
    uint64_t n_records;      /* records of the chunks                                                            */
    uint64_t n_compatible;   /* ... compatible with expected_ori (= n_routed + n_unrouted)                       */
    uint64_t n_routed;       /* ... whose b0 is a routing entry (= the sum of the counts)                        */
    uint64_t n_unrouted;     /* ... whose b0 is none                                                             */
    uint64_t n_long_records; /* records whose alignment words the whole wave tested out of global memory: more than
                                afq_gpl_multi_limits()[2] alignments, under fw / rc                              */
} afq_gpl_multi_hist_stats;
int afq_gpl_multi_hist_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t b0_bytes,
                           uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, const uint64_t* sample_observed,
                           uint64_t n_entries, uint64_t* out_n, uint32_t** out_entry, uint64_t** out_cell, uint64_t** out_count,
                           afq_gpl_multi_hist_stats* stats);
/* out[0] = bytes of a chunk the multi-barcode GPL parse stages per trip, out[1] = bytes staged behind them (they hold the widest
 * head, 4 + 4 + 4 + 8, and out[2] of the widest alignments), out[2] = a record with more alignments than this is a long record
 * (all three are afq_gpl_limits'), out[3] = 0.  For tests. */
void afq_gpl_multi_limits(uint32_t out[4]);

/*
 * `atac generate-permit-list`, the device half (update_barcode_hist_unfiltered, src/atac/cellfilter.rs:68-103 of the reference): one
 * walk of an UNCOLLATED scATAC RAD for the barcode histogram, the largest na and the position-bin histogram.
 *
 * `bytes` / `chunk_off` / bytes_on_device and the record layout (`na u32, barcode (bc_bytes), na x (ref u32, type u8, start_pos u32,
 * frag_len u16)`) are afq_atac_sort_rad's.  bin_base[ref_count + 1] ascends from bin_base[0] == 0 (else AFQ_ERR_INVALID_ARG):
 * reference r owns bins [bin_base[r], bin_base[r + 1]); bin_size >= 1.
 *
 * EVERY record counts its barcode, whatever its na, and max_ambig is the largest na over all records.  A record with exactly one
 * alignment adds 1 to bin bin_base[ref] + start_pos / bin_size.  No position is tested against a reference length - the reference
 * tests none - so a position past its reference's bins counts in the bins of the NEXT reference.  ref >= ref_count, or a bin index
 * >= bin_base[ref_count] (where the reference panics on an index), is AFQ_ERR_BAD_INPUT "chunk <i>: ...".
 *
 * Out (malloc'd; afq_free): the distinct barcodes, ascending, with their u64 counts; out_bins[bin_base[ref_count]] (NULL without
 * bins); `stats`.  All counts are integer sums: the output is a function of the input alone, run to run.  The counting table is
 * afq_gpl_hist_rad's, so afq_gpl_table_slot(barcode, n_records, bc_bytes, ..) describes it.  One call is one fill of the device: a
 * host with a larger file calls once per part, merges the sorted histograms, adds the bins and sums, takes the largest max_ambig.
 * Errors: AFQ_ERR_BAD_INPUT "chunk <i>: ..." for a chunk outside the buffer, a head or an alignment list that runs past its chunk,
 * records that do not tile nbytes or do not number nrec (nothing outside `bytes` is read, the context stays usable);
 * AFQ_ERR_UNSUPPORTED for 2^30 records or more in one call or 2^31 bins or more; AFQ_ERR_OOM (with the sizes) when input and
 * tables do not fit the device.
 */
typedef struct afq_atac_gpl_hist_stats {
    uint64_t n_records;      /* records of the chunks (= the sum of the barcode counts)        */
    uint64_t n_unmapped;     /* ... with na == 0                                              */
    uint64_t n_multimapped;  /* ... with na > 1                                               */
    uint64_t n_binned;       /* ... with na == 1 (= the sum of the bins)                      */
    uint64_t max_ambig;      /* the largest na over ALL records (`max-ambig-record`)          */
    uint64_t max_bin;        /* the largest bin counter (`max-rec-in-bin`); 0 without bins    */
} afq_atac_gpl_hist_stats;
int afq_atac_gpl_hist_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks,
                          uint32_t bc_bytes, int bytes_on_device, const uint64_t* bin_base /* [ref_count + 1] */, uint32_t ref_count,
                          uint32_t bin_size, uint64_t* out_n, uint64_t** out_bc, uint64_t** out_count, uint64_t** out_bins,
                          afq_atac_gpl_hist_stats* stats);
/* out[0] = bytes of a chunk the walk stages per trip, out[1] = bytes staged behind them (both are the `atac sort` parse's),
 * out[2] = bins a workgroup counts privately in LDS (0: the bins are counted in global memory), out[3] = 0.  For tests. */
void afq_atac_gpl_limits(uint32_t out[4]);

/*
 * `collate`, the device half (src/collate.rs:129-289, 483-643 of the reference): the records of an UNCOLLATED single-barcode RNA
 * RAD routed by corrected barcode into one chunk per cell.
 *
 * `bytes` / `chunk_off` / the record layout / expected_ori are afq_gpl_hist_rad's.  `observed` -> `corrected` is the correction
 * map (n_corrections entries; one observed barcode may occur twice only with one target); `cells` (n_cells, distinct) are the
 * output cells IN OUTPUT ORDER, and every corrected barcode must be one of them.
 *
 * A record is kept iff it is compatible with expected_ori (afq_gpl_hist_rad's rule, `na == 0` only under both) and its barcode
 * is an observed key.  It is written with the corrected barcode, its UMI, and ONLY the alignments that fit expected_ori (all of
 * them under both), in input order, each word untouched (bit 31 stays) with its position bytes; na becomes their number.
 *
 * Out (malloc'd; afq_free): out_bytes = the n_cells chunks back to back, each `nbytes u32, nrec u32` + its records, a cell
 * without a record being a header-only chunk (8, 0); out_chunk_off[n_cells + 1]; out_nrec[n_cells].  Inside a chunk the records
 * stand in input order (chunk index, then record index): the output is a function of the input alone, byte for byte.
 *
 * AFQ_ERR_BAD_INPUT: a chunk outside `bytes` or whose records do not tile it ("chunk i"), a corrected barcode that is no cell, two
 * targets for one observed barcode, two cells with one barcode.  AFQ_ERR_UNSUPPORTED: 2^32 records or more in one call, more than
 * 2^32 - 2 cells, 2^30 correction entries or more, an output chunk of 4 GiB or more (the cell is named).  AFQ_ERR_OOM (with the
 * sizes) when input, output, 32 bytes a record and the tables do not fit the device: one call is one device fill.
 */
typedef struct afq_collate_stats {
    uint64_t n_records;          /* records of the chunks                                                     */
    uint64_t n_compatible;       /* ... compatible with expected_ori                                          */
    uint64_t n_uncorrected;      /* ... of those, with a barcode that is not in the map                       */
    uint64_t n_kept;             /* records written (= n_compatible - n_uncorrected)                          */
    uint64_t n_alignments_in;    /* alignments of all records                                                 */
    uint64_t n_alignments_kept;  /* alignments written                                                        */
    uint64_t n_long_records;     /* records with more than afq_collate_limits()[2] alignments: the whole wave
                                    handles them out of global memory                                         */
    uint64_t out_bytes;          /* length of out_bytes                                                       */
} afq_collate_stats;
int afq_collate_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes,
                    uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, const uint64_t* observed, const uint64_t* corrected,
                    uint64_t n_corrections, const uint64_t* cells, uint64_t n_cells, uint8_t** out_bytes, uint64_t* out_n_bytes,
                    uint64_t** out_chunk_off, uint32_t** out_nrec, afq_collate_stats* stats);
/* out[0] = bytes of a chunk a collate walk stages per trip, out[1] = bytes staged behind them, out[2] = a record with more
 * alignments than this is a long record (all three are afq_gpl_limits'), out[3] = keys a workgroup of a radix pass takes.  For tests. */
void afq_collate_limits(uint32_t out[4]);

/*
 * multi-barcode `collate`, the device half (do_collate_multi_bc_fast, src/collate.rs:1415-1920 of the reference): the records
 * `na, b0, b1, umi, alignments` of an UNCOLLATED two-barcode RNA RAD routed to a sample by b0, corrected to a cell of that sample
 * by b1, and written as one chunk per cell.
 *
 * `bytes` / `chunk_off` / the record layout / expected_ori are afq_gpl_multi_hist_rad's; the context's aln_extra counts as there.
 * Three inputs, all in terms of a SAMPLE INDEX below n_samples (<= 2^31):
 *   sample table   sample_observed[i] (a b0 value, distinct) -> sample_index[i]                          (n_sample_entries)
 *   cell table     (corr_sample[i], corr_observed[i]) (distinct pairs) -> corr_corrected[i], which must be a cell of that sample
 *   cells          (cell_sample[j], cell_bc[j]) (distinct pairs) IN OUTPUT ORDER; sample_b0_out[s] is the value written into b0
 *                  for a record of sample s and must fit b0_bytes
 *
 * A record is kept iff it is compatible with expected_ori (afq_collate_rad's rule), its b0 is a key of the sample table, and its
 * b1 is an observed key of that sample.  It is written as na' = the number of fitting alignments, b0 = sample_b0_out[sample],
 * b1 = the corrected cell barcode, the UMI unchanged, and the fitting alignment words untouched in input order.
 *
 * Out: as afq_collate_rad - the n_cells chunks back to back (a cell without a record is a header-only chunk), out_chunk_off
 * [n_cells + 1], out_nrec[n_cells]; inside a chunk the records stand in input order, so the output is a function of the input alone.
 *
 * AFQ_ERR_INVALID_ARG: a null pointer, a width that is not 1, 2 or 4 (the UMI: 1, 2, 4 or 8), a bad expected_ori, a sample index
 * that is not below n_samples, n_samples above 2^31.  AFQ_ERR_BAD_INPUT: a value that does not fit its width, a duplicate key in
 * either table or among the cells, a correction into a barcode that is no cell of its sample, a chunk whose records do not tile it.
 * AFQ_ERR_UNSUPPORTED: a sample_b0_out value that does not fit b0_bytes, afq_collate_rad's size limits.  AFQ_ERR_OOM (with the
 * sizes) when input, output, 32 bytes a record and the tables do not fit the device: one call is one device fill.
 */
typedef struct afq_collate_multi_stats {
    uint64_t n_records;          /* records of the chunks                                                     */
    uint64_t n_compatible;       /* ... compatible with expected_ori                                          */
    uint64_t n_unrouted;         /* ... of those, with a b0 that is no key of the sample table                */
    uint64_t n_uncorrected;      /* ... routed, with a b1 that has no correction in that sample               */
    uint64_t n_kept;             /* records written (= n_compatible - n_unrouted - n_uncorrected)             */
    uint64_t n_alignments_in;    /* alignments of all records                                                 */
    uint64_t n_alignments_kept;  /* alignments written                                                        */
    uint64_t n_long_records;     /* records with more than afq_collate_multi_limits()[2] alignments           */
    uint64_t out_bytes;          /* length of out_bytes                                                       */
} afq_collate_multi_stats;
int afq_collate_multi_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t b0_bytes,
                          uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, const uint64_t* sample_observed,
                          const uint32_t* sample_index, uint64_t n_sample_entries, const uint32_t* corr_sample, const uint64_t* corr_observed,
                          const uint64_t* corr_corrected, uint64_t n_corrections, const uint32_t* cell_sample, const uint64_t* cell_bc, uint64_t n_cells,
                          const uint32_t* sample_b0_out, uint64_t n_samples, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off,
                          uint32_t** out_nrec, afq_collate_multi_stats* stats);
/* afq_collate_limits' four values, for the multi-barcode walks and the shared placement.  For tests. */
void afq_collate_multi_limits(uint32_t out[4]);

/*
 * `atac collate`, the device half (src/atac/collate.rs of the reference): the records of an UNCOLLATED scATAC RAD routed by
 * corrected barcode into one chunk per cell that receives a record.
 *
 * `bytes` / `chunk_off` / bytes_on_device / the record layout (`na u32, barcode (bc_bytes), na x (ref u32, type u8, start_pos u32,
 * frag_len u16)`) and `observed` -> `corrected` are afq_atac_sort_rad's; `cells` (n_cells, distinct) are the output cells IN OUTPUT
 * ORDER, and every corrected barcode must be one of them.
 *
 * A record is kept iff it has exactly one alignment and its barcode is an observed key: no orientation, map-type or range test
 * (collate.rs:719-723).  It is written as R = 4 + bc_bytes + 11 bytes: na = 1, the CORRECTED barcode, the 11 alignment bytes as read.
 *
 * Out (malloc'd; afq_free): out_bytes = one chunk (`nbytes u32, nrec u32` + its records) per cell that kept a record, in the order
 * of `cells` - a cell without a kept record is ABSENT; *out_n_chunks of them; out_chunk_off[n_out + 1]; out_nrec[n_out];
 * out_cell[n_out] = the index into `cells` of output chunk j.  Inside a chunk the records stand in input order (chunk index, then
 * record index): the output is a function of the input alone, byte for byte and run to run.
 *
 * AFQ_ERR_BAD_INPUT: a chunk outside `bytes`; records that do not tile nbytes or do not number nrec ("chunk i": nothing outside
 * `bytes` is read, the context stays usable); two targets for one observed barcode; a corrected barcode that is no cell; two cells
 * with one barcode.  AFQ_ERR_UNSUPPORTED: 2^32 records or more, more than 2^32 - 2 cells, 2^30 correction entries or more, an output
 * chunk of 4 GiB or more (the cell is named).  AFQ_ERR_OOM (with the sizes) when input, output, 20 bytes a record and the tables do
 * not fit the device: one call is one device fill.
 */
typedef struct afq_atac_collate_stats {
    uint64_t n_records;       /* records of the chunks                                   */
    uint64_t n_unmapped;      /* ... without an alignment                                */
    uint64_t n_multimapped;   /* ... with more than one                                  */
    uint64_t n_uncorrected;   /* ... with one alignment and a barcode not in the map     */
    uint64_t n_kept;          /* records written                                         */
    uint64_t n_cells_out;     /* chunks written: cells that kept a record                */
    uint64_t n_cells_empty;   /* cells that kept none (n_cells - n_cells_out)            */
    uint64_t out_bytes;       /* length of out_bytes                                     */
} afq_atac_collate_stats;
int afq_atac_collate_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes,
                         int bytes_on_device, const uint64_t* observed, const uint64_t* corrected, uint64_t n_corrections, const uint64_t* cells,
                         uint64_t n_cells, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t* out_n_chunks, uint64_t** out_chunk_off,
                         uint32_t** out_nrec, uint32_t** out_cell, afq_atac_collate_stats* stats);
/* out[0] = bytes of a chunk an `atac collate` walk stages per trip, out[1] = bytes staged behind them (both are the `atac sort`
 * parse's), out[2] = bytes of an alignment (11), out[3] = keys a workgroup of a radix pass takes.  For tests. */
void afq_atac_collate_limits(uint32_t out[4]);

/*
 * `convert`, the device half (bam2rad, src/convert.rs:167-594 of the reference): the alignment records of a BAM become the chunks
 * of a mapper RAD.  `bytes` is the INFLATED record stream behind the BAM header (host memory, or device memory when bytes_on_device);
 * span_off[n_spans] (host memory) are record starts, span_off[0] == 0, ascending: span i is [span_off[i], span_off[i + 1]), the
 * last one ends at n_bytes.  n_ref is the BAM header's reference count; bc_bytes / umi_bytes (1, 2, 4 or 8) are the widths of the
 * RAD's b and u fields.
 * A record whose flag has 0x4 or 0x800 does not exist for what follows.  The others are cut into runs of consecutive records with
 * byte-equal names; a run's barcode and UMI are the CR and UR strings of its first record, two bits a base (A0 C1 G2 T3, first base
 * most significant, one N as A, the low bc_bytes / umi_bytes bytes); a run with two N or more in either is dropped.  Every record
 * of a run is the alignment word refID | 0x80000000 (the bit when flag 0x10 is clear), in input order; with filter_best only the
 * records whose integer AS equals the run's largest.  A written run is `na:u32, b, u, na x u32`; 10 001 written runs make a chunk
 * `nbytes:u32, nrec:u32, records`, the last chunk holds the rest.
 * Out (malloc'd, freed with afq_free): the chunks back to back, out_chunk_off[n_chunks + 1] (the last entry: out_n_bytes),
 * out_nrec[n_chunks].  The output is a function of the input alone.
 * AFQ_ERR_BAD_INPUT "record <index in the stream>: ...": a block_size too small for the record's fixed fields, name, CIGAR and
 * sequence or past the span's end; aux fields that do not end at the record's end (scanned on run heads, and on every kept record
 * under filter_best); a kept record's refID outside [0, n_ref); a run head without CR / UR or with one not of type Z; a base outside
 * ACGTN in a written run; under filter_best a written run's record without an integer AS.  The context stays usable.
 * AFQ_ERR_UNSUPPORTED: 2^32 records or more, an output chunk of 4 GiB or more.  AFQ_ERR_OOM (with the sizes) when input and about
 * 120 bytes a kept record do not fit the device: one call is one device fill.  AFQ_ERR_INVALID_ARG: a null pointer, a bad width, a
 * span table that does not begin at 0, ascend and stay below n_bytes.
 */
typedef struct afq_convert_stats {
    uint64_t n_records;            /* records of the stream                                              */
    uint64_t n_dropped_by_flag;    /* ... with flag 0x4 or 0x800                                         */
    uint64_t n_runs;               /* runs of the other records                                          */
    uint64_t n_runs_dropped_n;     /* ... dropped for two N or more in CR or UR                          */
    uint64_t n_runs_written;
    uint64_t n_alignments_in;      /* records of the written runs                                        */
    uint64_t n_alignments_written; /* ... that were written (all of them without filter_best)            */
    uint64_t n_long_runs;          /* written runs of more than afq_convert_limits()[2] records: the whole wave takes them */
    uint64_t n_chunks;
    uint64_t out_bytes;            /* length of out_bytes                                                */
} afq_convert_stats;
int afq_convert_bam_rad(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const uint64_t* span_off, uint32_t n_spans, uint32_t n_ref, uint32_t bc_bytes,
                        uint32_t umi_bytes, int filter_best, int bytes_on_device, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off,
                        uint32_t** out_nrec, uint64_t* out_n_chunks, afq_convert_stats* stats);
/* out[0] = bytes of a span a convert walk stages per trip, out[1] = bytes staged behind them, out[2] = a run with more records
 * than this is taken by the whole wave, out[3] = flags a workgroup of the run-number and rank scans takes (the layout scan's take half as many).  For tests. */
void afq_convert_limits(uint32_t out[4]);

/* A snappy frame stream from `bytes`, compressed on the device (afq_snappy.hip): the 10-byte stream identifier, then one data
 * chunk per afq_snappy_limits()[0] bytes of input, in input order: `type, len24, masked CRC-32C of the uncompressed bytes`
 * and a raw snappy block (type 0x00), or the bytes themselves (type 0x01) wherever the raw block would not be shorter than
 * they are.  So n_out <= 10 + n_in + 8 n_blocks; empty input gives the identifier alone.  The stream is a function of the
 * input alone - the same bytes on every run and after any earlier call on the context - but not the bytes another snappy
 * encoder would write: no compressor promises that.  Chunks decode independently (no copy reaches across a chunk boundary).
 * bytes_on_device: `bytes` is a device pointer.  Input, slots (a worst-case raw block a chunk), stream and tables that do
 * not fit the device are refused with AFQ_ERR_OOM and the sizes before any launch.  out_bytes is malloc'd: afq_free. */
typedef struct afq_snappy_stats {
    uint64_t n_in, n_out;                          /* bytes in, bytes of the stream                  */
    uint64_t n_blocks, n_blocks_stored;            /* frame chunks; of those, written as type 0x01   */
    uint64_t n_literal_bytes, n_copies;            /* over the compressed chunks                     */
} afq_snappy_stats;
int afq_snappy_frame_encode(afq_ctx* ctx, const uint8_t* bytes, size_t n_bytes, int bytes_on_device, uint8_t** out_bytes, uint64_t* out_n_bytes,
                            afq_snappy_stats* stats);
/* out[0] = bytes of input per frame chunk (<= 65536), out[1] = slots of a chunk's last-position table, out[2] = longest single
 * copy element (<= 64), out[3] = chunks a workgroup takes.  For tests. */
void afq_snappy_limits(uint32_t out[4]);
/* The way back: the bytes of a snappy frame stream, decoded on the device (afq_snappy.hip, k_snappy_decode: one workgroup per
 * data chunk, the chunk built in LDS, its masked CRC-32C checked there).  `stream` is host memory; the host plans it by its
 * chunk headers and it crosses in pieces of whole chunks - at most afq_snappy_decode_limits()[2] data chunks, one launch a
 * piece, never more than two pieces of compressed bytes on the device.  shift (0..3): decoded byte x lies at (*out)[shift + x]
 * of the device buffer, whose base is 4-byte aligned at least.
 * out_on_device = 0: *out is malloc'd host memory holding the *out_n decoded bytes (afq_free).
 * out_on_device = 1: *out is device memory of the context, valid until the next decode on it or afq_destroy.
 * What the decoder has to allocate and the device does not have free is AFQ_ERR_OOM with the sizes before any allocation or launch.  A stream the plan refuses, a corrupt block and
 * a CRC mismatch are AFQ_ERR_BAD_INPUT with the host decoder's sentence ("corrupt snappy block", "snappy CRC mismatch", ...)
 * followed by "(chunk N ...)", N the lowest data chunk that is refused; nothing out of range is read or written for any body,
 * and the context serves again.  stats: n_in = n, n_out = *out_n, the rest as the encoder's over the stream's chunks. */
int afq_snappy_frame_decode_device(afq_ctx* ctx, const uint8_t* stream, size_t n, uint32_t shift, int out_on_device, uint8_t** out, uint64_t* out_n,
                                   afq_snappy_stats* stats);
/* out[0] = bytes of a chunk's body staged per trip, out[1] = threads of a workgroup (one data chunk each), out[2] = data chunks
 * of a launch at the most, out[3] = LDS bytes of a workgroup.  For tests. */
void afq_snappy_decode_limits(uint32_t out[4]);
/* The chunk table of a collated record stream that lies on the device (such as afq_snappy_frame_decode_device's output):
 * d_bytes is a device pointer of any alignment to n bytes, the first chunk's header stands at first_chunk, every chunk begins
 * with `nbytes:u32, nrec:u32` and the next one stands nbytes further.  One wave hops the headers (k_collated_chunk_table).
 * Outputs, malloc'd (afq_free), one entry a chunk: its offset, nbytes, nrec, and the 8 bytes at offset + 12 - the first record's
 * barcode field - little-endian, bytes behind the buffer's end as 0.  rec_hdr_bytes: the bytes of a record's head (na, barcode,
 * UMI); a chunk must hold one record at least; 0: that is not asked.  Refusals, AFQ_ERR_BAD_INPUT, at the first chunk they hold
 * for, with the sentences of afq_quantify's hop: "trailing bytes after the last chunk", "corrupt chunk header", "chunk N holds
 * no record". */
int afq_collated_chunk_table(afq_ctx* ctx, const uint8_t* d_bytes, uint64_t n, uint64_t first_chunk, uint32_t rec_hdr_bytes, uint64_t** off, uint32_t** nbytes,
                             uint32_t** nrec, uint64_t** first_bc, uint64_t* n_chunks);
/* on != 0: afq_collate_rad, afq_collate_multi_rad and afq_atac_collate_rad run as they do up to and including their write walk
 * and then hand out_bytes / out_n_bytes out as the snappy frame stream of the chunk bytes (afq_snappy_frame_encode's, encoded
 * where the bytes lie, in place of the plain copy down).  out_chunk_off, out_nrec, out_cell and every stats field, out_bytes
 * included, stay in uncompressed coordinates and equal the plain call's; the refusals and their words are the plain call's,
 * the memory plan counts the encoder's buffers.  0 (the default): nothing changes. */
void afq_set_collate_compress(afq_ctx* ctx, int on);

/* The bytes of a BGZF file (SAM/BAM specification 4.1: gzip members of at most 64 KiB with a BC extra field), inflated on the
 * device (afq_inflate.hip, k_bgzf_inflate: one workgroup per BGZF block, the block built in LDS from a raw deflate stream of
 * stored, fixed and dynamic blocks, its CRC-32 and ISIZE checked there).  `file` is host memory; the host plans it by its block
 * headers (the plan of afq_convert) and it crosses in pieces of whole blocks - at most afq_inflate_limits()[1] blocks, one launch
 * a piece, never more than two pieces of compressed bytes on the device.  shift (0..15): inflated byte x lies at
 * (*out)[shift + x] of the device buffer, whose base is 16-byte aligned.  Bytes behind a payload's final deflate block are
 * accepted, as zlib accepts them.
 * out_on_device = 0: *out is malloc'd host memory holding the *out_n inflated bytes (afq_free).
 * out_on_device = 1: *out is device memory of the context, valid until the next inflate on it or afq_destroy.
 * Compressed pieces, plan, status and inflated bytes that the inflater has to allocate and the device does not have free are
 * AFQ_ERR_OOM with the sizes before any allocation or launch.  A file the plan refuses is AFQ_ERR_BAD_INPUT with afq_convert's
 * sentence; so is a bad block: "BGZF block N: ", N the lowest block that is refused, and "bad CRC32", "ISIZE says I bytes, the
 * deflate stream holds P", or "the deflate stream is corrupt or longer than ISIZE (...)" with what the parser found; nothing out
 * of range is read or written for any payload, a refused block writes nothing, and the context serves again. */
typedef struct afq_inflate_stats {
    uint64_t n_in, n_out;                   /* bytes of the file, bytes inflated               */
    uint64_t n_blocks, n_blocks_empty;      /* BGZF blocks; of those with ISIZE 0              */
    uint64_t n_stored, n_fixed, n_dynamic;  /* deflate blocks by type                          */
    uint64_t n_literals, n_copies;          /* over fixed and dynamic blocks                   */
} afq_inflate_stats;
int afq_bgzf_inflate_device(afq_ctx* ctx, const uint8_t* file, size_t n, uint32_t shift, int out_on_device, uint8_t** out, uint64_t* out_n,
                            afq_inflate_stats* stats);
/* out[0] = threads of a workgroup, out[1] = BGZF blocks of a launch at the most, out[2] = LDS bytes of a workgroup, out[3] =
 * blocks a workgroup takes.  For tests. */
void afq_inflate_limits(uint32_t out[4]);

/*
 * Kernel timing of the last collected batch (HIP events on the context's own
 * stream; only when cfg.profile != 0).  Fills up to `cap` entries; returns the
 * number of kernels, or a negative error.  `name[i]` points to static storage.
 */
typedef struct afq_kernel_time {
    const char* name;
    double ms;       /* summed over launches   */
    uint32_t launches;
    uint32_t pad;
} afq_kernel_time;
int afq_get_kernel_times(afq_ctx* ctx, afq_kernel_time* out, uint32_t cap);

/* Number of records / keys the last collected batch processed (for the bench's byte model). */
typedef struct afq_batch_stats {
    uint64_t n_records;
    uint64_t n_ref_words;  /* sum of na                                            */
    uint64_t n_keys;       /* (umi,gene) pairs after per-read gene dedup           */
    uint64_t n_buckets;
    uint64_t n_overflow_buckets;
    uint64_t input_bytes;
    uint64_t n_fallback_cells; /* cells the walk-free decode could not prove and re-decoded sequentially */
} afq_batch_stats;
int afq_get_batch_stats(afq_ctx* ctx, afq_batch_stats* out);
/* Parsimony: labels of three or more ids are keyed by a 62-bit hash; two different labels of one cell under one key are
   detected on the device, and the range of cells is then decoded again with another hash function instead of being refused
   (the reference keys its map by the list itself, eq_class.rs:859-903).  How often that happened since afq_create. */
uint64_t afq_label_rehash_count(const afq_ctx* ctx);
/* Parsimony: the per-cell graphs are built in a pool sized by the range's reads (24 words per read).  A range whose graphs
   outgrow it (short UMIs: hundreds of reads per UMI, so a vertex has many neighbours) is run again with four times the pool,
   up to three times, or - when the device has no room for that - in halves, down to a single cell with four times a pool of
   its own, before AFQ_ERR_OOM (the reference allocates per graph, pugutils.rs:65-267).  How often a range (or a part of one)
   failed that way since afq_create. */
uint64_t afq_pool_regrow_count(const afq_ctx* ctx);
/* EM resolutions: ranges whose EM did not fit the device scratch set aside for it ahead of time and was sized on the host
 * instead (one extra trip to the host for that range; results identical).  Diagnostics only. */
uint64_t afq_em_resize_count(const afq_ctx* ctx);
/* Parsimony: cells resolved by the one-workgroup kernel instead of the partition-parallel phase kernels - sent there directly
 * (gene-level parsimony, 8-byte UMIs) or handed back (a UMI partition of more than 256 reads; a component of more than 4096
 * vertices under a --large-graph-thresh raised beyond that).  Results identical; diagnostics only. */
uint64_t afq_mono_cell_count(const afq_ctx* ctx);
/* cr-like / cr-like-em: buckets of the last collected batch that the hash resolve handed to the sort path - single-bucket cells,
 * buckets of 257..512 keys, and buckets whose UMIs the hash table cannot hold (a UMI over 32 bits, more than eight genes or 64
 * parked keys).  Batches that the table never serves (prefer-ambig, trivial, cr-like-em of many-gene reads) are sorted without
 * a hash pass and count 0.  Results identical; diagnostics only. */
uint64_t afq_resolve_divert_count(const afq_ctx* ctx);
/* EM resolutions: cells of the last collected batch per instance of the order-free EM's rounds kernel (afq_em2.hip):
 * out[0..2] everything in LDS at 256 / 512 / 1024 threads, out[3] class lists streamed, out[4] the hot entries in LDS and the
 * rest in global memory; out[5] those of out[4] that ran with 32-bit state ids.  Cells without an ambiguous molecule, and
 * batches under AFQ_EM_ORDER=canonical (the sequential kernels of afq_em.hip), count nowhere.  Diagnostics only. */
void afq_em_instance_counts(const afq_ctx* ctx, uint64_t out[6]);
/* The range pipeline of the last submitted batch: out[0] its ranges, out[1] those whose rows went onto the copy stream without
 * the host waiting for them (waited for in afq_collect), out[2] those that first let the copy stream drain and then waited for
 * their own rows (a range run again, rows beyond the slot's row buffers, EM resolutions, an error), out[3] how often the
 * result arrays had to grow while rows were crossing into them, which waits for those rows.  out[1] + out[2] counts the
 * ranges finished so far (all of them after afq_collect).  Diagnostics only. */
void afq_range_pipeline_counts(const afq_ctx* ctx, uint64_t out[4]);

/* Brings the HIP runtime up on `device` (first-call initialisation) - a host can call it from a side thread while it parses its
   inputs.  Returns 0 or AFQ_ERR_NO_DEVICE. */
int afq_device_warmup(int device);
/* PCI bus id of `device` ("0000:c1:00.0"), for a host that wants to place its threads and buffers on the device's NUMA node
   (/sys/bus/pci/devices/<id>/numa_node).  Returns 0, AFQ_ERR_NO_DEVICE or AFQ_ERR_INVALID_ARG (out too small). */
int afq_device_pci_bus_id(int device, char* out, size_t out_len);

const char* afq_last_error(const afq_ctx* ctx); /* ctx may be NULL: last create error */
int afq_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* AFQUANT_H */
