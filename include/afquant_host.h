/*
 * afquant_host.h — the host side around the quant hot path, in C++ because the
 * reference's host is compiled code and this image has no Rust toolchain.  It mirrors what
 * `alevin_fry::quant::quantify(QuantOpts)` does around the per-cell loop (src/quant.rs:359-396,
 * 1327-1951 of the reference): read `collate.json`, open `map.collated.rad[.sz]`, parse the RAD
 * prelude and the transcript-to-gene map, feed the collated chunks to the device through afquant.h,
 * and write `alevin/quants_mat.{mtx,_rows.txt,_cols.txt}`, `featureDump.txt` and `quant.json`.
 */
#ifndef AFQUANT_HOST_H
#define AFQUANT_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

struct afq_atac_stats;

/* QuantOpts (src/prog_opts.rs:24-44) — the CLI-visible options of `alevin-fry quant` (src/main.rs:294-348). */
typedef struct afq_quant_opts {
    const char* input_dir;      /* -i : directory holding map.collated.rad[.sz], collate.json, generate_permit_list.json */
    const char* tg_map;         /* -m : 2- or 3-column transcript-to-gene TSV                                             */
    const char* output_dir;     /* -o                                                                                      */
    const char* resolution;     /* -r : trivial | cr-like | cr-like-em | parsimony | parsimony-em | parsimony-gene | parsimony-gene-em */
    const char* filter_list;    /* --quant-subset : file of barcodes to quantify, or NULL                                  */
    const char* cmdline;        /* recorded in quant.json                                                                  */
    uint32_t num_threads;       /* -t : accepted for compatibility; the device does the per-cell work                      */
    uint32_t small_thresh;      /* --small-thresh (default 100)                                                            */
    int32_t umi_edit_dist;      /* --umi-edit-dist : -1 = default by resolution (main.rs:652-703)                          */
    int32_t large_graph_thresh; /* --large-graph-thresh : -1 = default by resolution (main.rs:332-341)                     */
    uint32_t init_uniform;      /* --init-uniform                                                                          */
    uint32_t dump_eq;           /* -d : also write geqc_counts.mtx + gene_eqclass.txt.gz (quant.rs:229-355)                */
    uint32_t num_bootstraps;    /* -b : bootstrap replicates; writes bootstraps_mean.mtx + bootstraps_var.mtx (quant.rs:1850-1877) */
    uint32_t device;            /* HIP device ordinal                                                                      */
    uint64_t batch_bytes;       /* chunk bytes handed to a device per afq_submit (0 = 16 GiB; a batch is pipelined internally) */
    uint32_t sa_model;          /* --sa-model (hidden): afq_sa_model; ignored with a log line outside USA mode (quant.rs:1456) */
    uint32_t summary_stat;      /* --summary-stat (requires -b)                                                            */
    uint64_t boot_seed;         /* seed of the bootstrap draws (the reference's are unseeded); --boot-seed, default 0     */
    const int32_t* devices;     /* --devices 0,1,... : HIP device ordinals to spread the cells over (NULL / 0 = just `device`).  The
                                   worker fan-out of do_quantify (quant.rs:1553-1575, 1678-1765): one context and one host thread
                                   per device over a contiguous, byte-balanced range of cells; rows are gathered in cell order, so
                                   the output does not depend on the device count                                          */
    uint32_t n_devices;
    uint32_t sz_on_device;      /* --sz-on-device : map.collated.rad.sz is decoded on the device (afq_snappy_frame_decode_device) and stays there -
                                   the prelude comes from its leading frame chunks, the chunk table from afq_collated_chunk_table, the
                                   batches are submitted where the decoder left them.  One device only (several: AFQ_ERR_UNSUPPORTED);
                                   ignored with a log line when the directory is not compressed.  0: the file is decoded on the host   */
} afq_quant_opts;

/* The CLI-visible options of `alevin-fry infer` (src/main.rs:350-365). */
typedef struct afq_infer_opts {
    const char* count_mat;      /* -c : cells x equivalence classes, MatrixMarket (`geqc_counts.mtx` of `quant -d`); the barcode and
                                        gene-name files are looked up next to it (quants_mat_rows.txt, quants_mat_cols.txt)        */
    const char* eq_labels;      /* -e : gene_eqclass.txt.gz                                                                */
    const char* output_dir;     /* -o                                                                                      */
    const char* filter_list;    /* --quant-subset, or NULL                                                                 */
    uint32_t usa_mode;          /* --usa                                                                                   */
    uint32_t num_threads;       /* -t : threads of the MTX writer                                                          */
    uint32_t device;
    uint32_t reserved;
} afq_infer_opts;
/* Runs the whole `infer` sub-command (src/infer.rs:31-426): quants_mat.mtx, quants_mat_rows.txt, quants_mat_cols.txt in output_dir. */
int afq_infer_files(const afq_infer_opts* opts);

/* The options of `alevin-fry atac deduplicate` (src/atac/prog_opts.rs:47-55, src/main.rs:942-956). */
typedef struct afq_atac_dedup_opts {
    const char* input_dir;      /* -i : directory holding collate.json, generate_permit_list.json, map.collated.rad[.sz]; map.bed is written here */
    uint32_t num_threads;       /* -t : BED formatting / snappy threads (0 = all cores)                                   */
    uint32_t rev;               /* -d/--permit-bc-ori rc (the CLI default) : barcodes are written reverse-complemented    */
    uint32_t device;
    uint32_t sz_on_device;      /* --sz-on-device : as afq_quant_opts.sz_on_device                                        */
    struct afq_atac_stats* stats_out; /* optional: the counters the reference logs (deduplicate.rs:285-308)               */
} afq_atac_dedup_opts;
/* Runs the whole `atac deduplicate` sub-command (src/atac/deduplicate.rs:68-309) on the device: <input_dir>/map.bed. */
int afq_atac_deduplicate(const afq_atac_dedup_opts* opts);

/* The options of `alevin-fry atac sort` (src/main.rs:924-938). */
struct afq_atac_sort_stats;
typedef struct afq_atac_sort_opts {
    const char* input_dir;      /* -i : output directory of `atac generate-permit-list`; map.bed[.gz], sort.json and
                                        unmapped_bc_count_collated.bin are written here                                    */
    const char* rad_dir;        /* -r : the mapper's directory: map.rad, unmapped_bc_count.bin                             */
    uint32_t num_threads;       /* -t : BED formatting threads (0 = all cores)                                            */
    uint32_t compress;          /* -c : map.bed.gz instead of map.bed                                                     */
    uint32_t max_records;       /* -m : accepted and ignored (it sizes the reference's host buffers)                      */
    uint32_t device;
    const char* cmdline;        /* optional: goes into sort.json                                                          */
    struct afq_atac_sort_stats* stats_out;   /* optional */
} afq_atac_sort_opts;
/* Runs the whole `atac sort` sub-command (src/atac/sort.rs:170-895): the coordinate-sorted, de-duplicated BED of an uncollated RAD. */
int afq_atac_sort(const afq_atac_sort_opts* opts);

/* The options of `alevin-fry collate` (src/main.rs:271-292) for single-barcode RNA RAD files. */
struct afq_collate_stats;
typedef struct afq_collate_opts {
    const char* input_dir;      /* -i : output directory of `generate-permit-list`; map.collated.rad, collate.json and
                                        unmapped_bc_count_collated.bin are written here                                    */
    const char* rad_dir;        /* -r : the mapper's directory: map.rad, unmapped_bc_count.bin (optional)                  */
    uint32_t num_threads;       /* -t : accepted; the device routes the records                                           */
    uint32_t compress;          /* -c : refused (AFQ_ERR_UNSUPPORTED) by this entry, ignored by the _sz entry below        */
    uint32_t max_records;       /* -m : accepted, without effect (it sizes the reference's host buffers)                   */
    uint32_t device;
    const char* cmdline;        /* optional: goes into collate.json                                                        */
    struct afq_collate_stats* stats_out;   /* optional */
} afq_collate_opts;
/* Runs the whole `collate` sub-command (src/collate.rs:129-289, 483-643) in ONE device fill: one chunk per cell of permit_freq.bin,
 * in the order (count descending, barcode ascending); records barcode-corrected and cut to the alignments that fit expected_ori;
 * input order inside a chunk.  ATAC, multi-barcode and long-read preludes, multi_barcode / velo_mode metadata and compressed output
 * are AFQ_ERR_UNSUPPORTED, named in the message; a kept count other than the sum of permit_freq.bin is the reference's
 * "expected to collate N records but retained M", and no RAD is left behind. */
int afq_collate(const afq_collate_opts* opts);
/* `collate -c` (collate.rs:523-554): afq_collate with compressed output, through a door of its own - afq_collate and the command
 * line's -c keep answering "compressed output is not supported", word for word, because the tests that pin that refusal are
 * not changed here; a follow-up that may touch them retires it in one line.  opts->compress is ignored.  Writes
 * map.collated.rad.sz in place of map.collated.rad: the snappy frame stream of the prelude (num_chunks patched), then the frame
 * stream of the chunks - two streams back to back, each with its identifier, as the reference's own file is and as
 * afq_quantify / afq_atac_deduplicate read it - both compressed on the device (afq_snappy_frame_encode; the chunks where the
 * write walk left them, afq_set_collate_compress); collate.json with "compressed_output": true; unmapped_bc_count_collated.bin
 * as afq_collate.  Everything else, the refusals and the kept-count check that leaves no file behind included, is afq_collate's. */
int afq_collate_sz(const afq_collate_opts* opts);

/* The options of `alevin-fry atac collate` (src/main.rs:905-922). */
struct afq_atac_collate_stats;
typedef struct afq_atac_collate_opts {
    const char* input_dir;      /* -i : output directory of `atac generate-permit-list`; map.collated.rad, collate.json and
                                        unmapped_bc_count_collated.bin are written here                                    */
    const char* rad_dir;        /* -r : the mapper's directory: map.rad, unmapped_bc_count.bin (optional)                  */
    uint32_t num_threads;       /* -t : accepted; the device routes the records                                           */
    uint32_t compress;          /* -c : refused (AFQ_ERR_UNSUPPORTED) by this entry, ignored by the _sz entry below        */
    uint32_t max_records;       /* -m : accepted, without effect (it sizes the reference's host buffers)                   */
    uint32_t device;
    const char* cmdline;        /* optional: goes into collate.json                                                        */
    struct afq_atac_collate_stats* stats_out;   /* optional */
} afq_atac_collate_opts;
/* Runs the whole `atac collate` sub-command (src/atac/collate.rs) in ONE device fill: the first `num-chunks` chunks of map.rad; one
 * chunk per cell of permit_freq.bin THAT KEPT A RECORD, in the order (count descending, barcode ascending); a record is kept iff it
 * has one alignment and its barcode is in the correction map; input order inside a chunk; the header's num_chunks is the number of
 * chunks written.  An RNA prelude and compressed output are AFQ_ERR_UNSUPPORTED.  A missing unmapped_bc_count.bin is an empty map
 * (the reference panics).  map.collated.rad is written only after the device call succeeded: a failed run leaves none behind. */
int afq_atac_collate(const afq_atac_collate_opts* opts);
/* `atac collate -c`: afq_atac_collate writing map.collated.rad.sz, as afq_collate_sz does for afq_collate (opts->compress is
 * ignored; afq_atac_collate itself keeps its refusal).  With no record kept the chunk stream is the identifier alone. */
int afq_atac_collate_sz(const afq_atac_collate_opts* opts);

/* The options of multi-barcode `collate` (src/main.rs:271-292; do_collate_multi_bc_fast, src/collate.rs:1415-1920): afq_collate_opts'
 * fields, over the output directory of afq_generate_permit_list_multi. */
struct afq_collate_multi_stats;
typedef struct afq_collate_multi_opts {
    const char* input_dir;      /* -i : output directory of multi-barcode `generate-permit-list` (generate_permit_list.json,
                                        sample_info.json, sample_<name>/permit_freq.bin, correction_plan.bin); map.collated.rad,
                                        collation_manifest.bin, collate.json and unmapped_bc_count_collated.bin are written here  */
    const char* rad_dir;        /* -r : the mapper's directory: map.rad                                                     */
    uint32_t num_threads;       /* -t : accepted; the device routes the records                                           */
    uint32_t compress;          /* -c : refused (AFQ_ERR_UNSUPPORTED) by this entry, ignored by the _sz entry below        */
    uint32_t max_records;       /* -m : accepted, without effect                                                          */
    uint32_t device;
    const char* cmdline;        /* optional: goes into collate.json                                                        */
    struct afq_collate_multi_stats* stats_out;   /* optional */
} afq_collate_multi_opts;
/* Runs multi-barcode `collate` in ONE device fill: one chunk per (sample, cell) of the samples' permit_freq.bin files, in the order
 * (position in sample_info.json's samples, count descending, barcode ascending); a record is kept iff it is compatible with
 * expected_ori, its b0 is an observed key of the plan's sample corrections whose target is a sample of sample_info.json, and its b1
 * is an observed key of that sample's cell scope; it is written with b0 = the dense ordinal of the sample among the samples that
 * have cells and b1 = the corrected cell barcode.  collation_manifest.bin holds one group per sample with cells;
 * unmapped_bc_count_collated.bin is the empty map.  Metadata without multi_barcode: true, velo_mode, a single-barcode or scATAC
 * prelude, a pos tag, more than two barcode levels, an ordinal that does not fit b0, compressed output and a MISSING
 * correction_plan.bin are AFQ_ERR_UNSUPPORTED; a plan that is malformed, not sample-scoped or of another cell barcode length, a
 * sample with cells and no cell scope, and a correction into a barcode that is no cell of its sample are AFQ_ERR_BAD_INPUT.  Per
 * sample the records kept must number the sum of its permit_freq.bin counts ("expected to collate N records but retained M");
 * the files are written only after that check, so a failed run leaves none behind. */
int afq_collate_multi(const afq_collate_multi_opts* opts);
/* multi-barcode `collate -c`: afq_collate_multi writing map.collated.rad.sz, as afq_collate_sz does for afq_collate
 * (opts->compress is ignored; afq_collate_multi itself keeps its refusal).  collate.json's other keys and
 * collation_manifest.bin - it counts chunks, not bytes - are unchanged. */
int afq_collate_multi_sz(const afq_collate_multi_opts* opts);
/* afq_collate_multi_rad's checks that precede device work (include/afquant.h), without a device. */
int afq_collate_multi_check_args(uint32_t b0_bytes, uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, const uint64_t* sample_observed,
                                 const uint32_t* sample_index, uint64_t n_sample_entries, const uint32_t* corr_sample, const uint64_t* corr_observed,
                                 const uint64_t* corr_corrected, uint64_t n_corrections, const uint32_t* cell_sample, const uint64_t* cell_bc, uint64_t n_cells,
                                 const uint32_t* sample_b0_out, uint64_t n_samples);
/* collation_manifest.bin as afq_collate_multi writes it and afq_quantify reads it: level names sample, cell; one named group per
 * entry.  Returns the length; writes when out holds it (out may be NULL to size). */
int64_t afq_collation_manifest_bytes(const uint64_t* key, const char* const* name, const uint64_t* chunk_start, const uint64_t* num_chunks,
                                     const uint64_t* num_records, uint64_t n_groups, uint8_t* out, size_t cap);

/* The options of `alevin-fry generate-permit-list` (src/main.rs:170-269, 392-577; GenPermitListOpts, src/prog_opts.rs:86-160) for
 * single-barcode RNA RAD files.  Exactly one filter method is given. */
enum { AFQ_GPL_KNEE = 0, AFQ_GPL_EXPECT = 1, AFQ_GPL_FORCE = 2, AFQ_GPL_VALID_BC = 3, AFQ_GPL_UNFILTERED = 4 };
typedef struct afq_gpl_opts {
    const char* input_dir;      /* -i : directory holding the mapper's map.rad                                             */
    const char* output_dir;     /* -o                                                                                      */
    uint32_t expected_ori;      /* -d : 0 both / either, 1 fw, 2 rc                                                        */
    uint32_t method;            /* AFQ_GPL_*: -k, -e N, -f N, -b FILE, -u FILE                                             */
    uint64_t method_count;      /* N of -e / -f                                                                            */
    const char* list_file;      /* FILE of -b / -u                                                                         */
    uint64_t min_reads;         /* -m (with -u; at least 1)                                                                */
    uint32_t frequency;         /* --cell-bc-correction frequency (else unique)                                            */
    int32_t neighborhood;       /* --cell-bc-neighborhood: -1 = by method (prog_opts.rs:135-144), 0 hamming-1, 1 substitution-or-shift-1 */
    uint64_t conf_num, conf_den;/* --cell-bc-confidence, reduced (afq_gpl_parse_confidence); 0/0 = 39/40                   */
    uint32_t num_threads;       /* -t : recorded in generate_permit_list.json; the device reads the records                */
    uint32_t device;
    const char* cmdline;        /* recorded in generate_permit_list.json                                                   */
    uint64_t fill_bytes;        /* chunk bytes per device fill (0 = 8 GiB); a larger map.rad is read in several fills whose
                                   sorted histograms are merged                                                            */
    uint64_t* corrected_out;    /* optional: the number of distinct corrected barcodes                                     */
} afq_gpl_opts;
/* Runs the whole sub-command: permit_freq.bin, all_freq.bin (filtered methods), permit_map.bin, correction_plan.bin and
 * generate_permit_list.json in output_dir.  ATAC and multi-barcode preludes are AFQ_ERR_UNSUPPORTED, named in the message. */
int afq_generate_permit_list(const afq_gpl_opts* opts);

/* ---- generate-permit-list pieces for the CPU tests (no GPU needed) ---- */
/* Confidence::from_str (barcode_correction.rs:166-197): a decimal of at most 18 fractional digits or `a/b`, reduced exactly. */
int afq_gpl_parse_confidence(const char* text, uint64_t* num, uint64_t* den);
/* A barcode list file's text.  unfiltered != 0 (-u, cellfilter.rs:77-106): every line has one length (else an error), a line that is
 * not a full valid k-mer contributes nothing, *first_len receives the length of the first line.  unfiltered == 0 (-b,
 * cellfilter.rs:1832-1847): the first valid barcode_len-mer of every line; a line without one is an error.  Returns the number of
 * barcodes (file order, duplicates kept) or a negative error; out may be NULL to size, else at most cap are written. */
int64_t afq_gpl_parse_barcode_list(const uint8_t* text, size_t n, int unfiltered, uint32_t barcode_len, uint64_t* out, size_t cap, uint32_t* first_len);
/* get_knee (knee_finding.rs:99-139) of descending frequencies, in double without contraction; the reference's panics are
 * AFQ_ERR_BAD_INPUT with its sentence. */
int64_t afq_gpl_knee(const uint64_t* freq_desc, size_t n);
/* select_retained_barcodes (cellfilter.rs:740-780) for AFQ_GPL_KNEE / EXPECT / FORCE / UNFILTERED (threshold = arg) over a histogram
 * with ascending barcodes; writes the retained barcodes ascending (at most cap), returns their number or a negative error. */
int64_t afq_gpl_select_retained(const uint64_t* bc, const uint64_t* count, size_t n, uint32_t method, uint64_t arg, uint64_t* out, size_t cap);
/* The five output files from finished tables (all lists ascending by their first column): freq = permit_freq.bin's map,
 * all_freq (NULL: not written), map = permit_map.bin's pairs, plan = correction_plan.bin's entries; stats[8] in CorrectionStats order. */
typedef struct afq_gpl_tables {
    uint32_t barcode_len, neighborhood, frequency; uint32_t filtered;
    uint64_t conf_num, conf_den, pseudocount;
    const uint64_t *freq_bc, *freq_count; uint64_t n_freq;
    const uint64_t *all_bc, *all_count; uint64_t n_all;
    const uint64_t *map_obs, *map_cor; uint64_t n_map;
    const uint64_t *plan_obs, *plan_cor; uint64_t n_plan;
    uint64_t stats[8];
    uint64_t max_ambig;
} afq_gpl_tables;
int afq_gpl_write_outputs(const afq_gpl_opts* opts, const afq_gpl_tables* t);

/* The options of `alevin-fry atac generate-permit-list` (src/main.rs; the ATAC GenPermitListOpts, src/atac/prog_opts.rs:11-28). */
struct afq_atac_gpl_hist_stats;
typedef struct afq_atac_gpl_opts {
    const char* input_dir;      /* -i : directory holding the mapper's map.rad                                   */
    const char* output_dir;     /* -o                                                                            */
    const char* list_file;      /* -u : unfiltered external permit list, plain or gzip (required: the reference's
                                        only filter method, atac/cellfilter.rs:158-166)                          */
    uint64_t min_reads;         /* -m : the reference's CLI default is 10; < 1 is AFQ_ERR_INVALID_ARG with its sentence */
    uint32_t rc;                /* -d : 1 = rc (the reference's default), 0 = fw                                 */
    uint32_t num_threads;       /* recorded in the json                                                          */
    uint32_t frequency;         /* --cell-bc-correction: 0 unique, 1 frequency (pseudocount 1)                   */
    uint32_t neighborhood;      /* 0 hamming-1 (the ATAC default), 1 substitution-or-shift-1                      */
    uint64_t conf_num, conf_den;/* 0/0 = Confidence::ATAC = 9/10                                                 */
    uint32_t device;
    uint64_t fill_bytes;        /* 0 = 8 GiB; a device fill is a run of whole chunks of at most this many bytes   */
    const char* cmdline;
    struct afq_atac_gpl_hist_stats* stats_out;   /* may be NULL */
} afq_atac_gpl_opts;
/* Runs the whole sub-command (generate_permit_list + process_unfiltered, src/atac/cellfilter.rs): permit_freq.bin, permit_map.bin
 * (the plan's entries, NOT the theoretical neighbourhood), correction_plan.bin, bin_recs.bin, bin_lens.bin and
 * generate_permit_list.json in output_dir, every map in ascending key order.  The record pass runs fill by fill on the device
 * (afq_atac_gpl_hist_rad), the correction decisions are afq_gpl_correct's.  Listed barcodes are reverse-complemented under rc; the
 * retained ones are the listed with an exact count >= min_reads.  An RNA prelude is AFQ_ERR_UNSUPPORTED; reference lengths that
 * give no bin at all are AFQ_ERR_BAD_INPUT "bins should not be empty" (the reference panics with these words).  This is the
 * library entry point: the command-line word `atac generate-permit-list` is still refused by the CLI. */
int afq_atac_generate_permit_list(const afq_atac_gpl_opts* opts);
/* initialize_rec_list (atac/cellfilter.rs:39-54): out[n + 1] with out[0] = 0, out[r + 1] = out[r] + ceil((f32)ref_lens[r] / (f32)bin_size),
 * quotient and ceiling in f32 as the reference computes them.  For the CPU tests. */
void afq_atac_gpl_bin_lens(const uint32_t* ref_lens, size_t n, uint64_t bin_size, uint64_t* out);
/* needletail's reverse_complement of a packed k-mer (k = 1..32).  For the CPU tests. */
uint64_t afq_gpl_reverse_complement(uint64_t barcode, uint32_t k);

/* The options of `alevin-fry generate-permit-list` on a multi-barcode (10x Flex) RAD file (do_generate_permit_list_multi_bc,
 * src/cellfilter.rs:789-1381; GenPermitListOpts, src/prog_opts.rs:86-184).  The cell-side fields are afq_gpl_opts'; the cell
 * neighbourhood's default (-1) is hamming-1 here (resolved_cell_neighborhood(true)). */
enum { AFQ_GPL_SAMPLE_EXACT = 0, AFQ_GPL_SAMPLE_UNIQUE = 1, AFQ_GPL_SAMPLE_FREQUENCY = 2, AFQ_GPL_SAMPLE_ONE_EDIT = 3 };
struct afq_gpl_multi_hist_stats;
typedef struct afq_gpl_multi_opts {
    const char* input_dir;      /* -i : directory holding the mapper's map.rad                                             */
    const char* output_dir;     /* -o                                                                                      */
    uint32_t expected_ori;      /* -d : 0 both / either, 1 fw, 2 rc                                                        */
    uint32_t method;            /* AFQ_GPL_*: -k, -e N, -f N, -b FILE, -u FILE                                             */
    uint64_t method_count;      /* N of -e / -f                                                                            */
    const char* list_file;      /* FILE of -b / -u (with -u: the cell-barcode whitelist that splits every sample's histogram) */
    uint64_t min_reads;         /* -m (with -u; at least 1)                                                                */
    uint32_t frequency;         /* --cell-bc-correction frequency (else unique)                                            */
    int32_t neighborhood;       /* --cell-bc-neighborhood: -1 = hamming-1, 0 hamming-1, 1 substitution-or-shift-1          */
    uint64_t conf_num, conf_den;/* --cell-bc-confidence; 0/0 = 39/40                                                       */
    uint32_t num_threads;       /* -t : the device reads the records                                                       */
    uint32_t device;
    const char* cmdline;        /* recorded in generate_permit_list.json                                                   */
    uint64_t fill_bytes;        /* chunk bytes per device fill (0 = 8 GiB); the sorted outputs of several fills are merged */
    const char* sample_bc_list; /* --sample-bc-list (required): one, two or three tab-separated columns                    */
    uint32_t sample_correction; /* --sample-bc-correction: AFQ_GPL_SAMPLE_*; ONE_EDIT is the deprecated `1-edit`: unique
                                   over substitution-or-shift-1, whatever sample_neighborhood says (prog_opts.rs:161-184)  */
    uint32_t sample_neighborhood;        /* --sample-bc-neighborhood: 0 hamming-1 (the default), 1 substitution-or-shift-1 */
    uint64_t sample_conf_num, sample_conf_den;   /* --sample-bc-confidence; 0/0 = 39/40                                    */
    uint32_t sample_bc_ori;     /* --sample-bc-ori: 0 forward, 1 reverse (both columns are reverse-complemented)           */
    struct afq_gpl_multi_hist_stats* stats_out;   /* optional: the record pass's stats, summed over the fills               */
} afq_gpl_multi_opts;
/* Runs the whole step: sample_permit_map.bin, sample_<name>/permit_map.bin and sample_<name>/permit_freq.bin (none for a sample
 * without a read: it gets its directory and its sample_info entry), correction_plan.bin with a sample scope and one cell scope per
 * sample, sample_info.json (the reference's keys; the three *_seconds keys and correction_plan_bytes hold what was measured here,
 * the four spill_* keys are 0: there is no spool) and generate_permit_list.json in output_dir, every map in ascending key order.
 * The record pass runs fill by fill on the device (afq_gpl_multi_hist_rad) over the routing entries - the exact sources, the
 * structurally unique neighbours and, under frequency, the structurally ambiguous barcodes, whose pairs the host replays once the
 * exact counts are known; the cell correction of every sample is afq_gpl_correct's.  Returns total_cells (the sum of the samples'
 * permitted cells) or a negative AFQ_ERR_* code.  A single-barcode or scATAC prelude, more than two barcode levels and alignment
 * positions are AFQ_ERR_UNSUPPORTED, named in the message.  This is the library entry point: `afquant generate-permit-list
 * --sample-*` is still refused by the CLI, and afq_generate_permit_list still refuses a multi-barcode prelude. */
int64_t afq_generate_permit_list_multi(const afq_gpl_multi_opts* opts);
/* ---- multi-barcode generate-permit-list pieces for the CPU tests (no GPU needed) ---- */
/* load_sample_barcode_list (cellfilter.rs:1405-1569) of a file's text, then build_sample_permit_map (1581-1666) under
 * sample_correction / sample_neighborhood: the routing entries the device call gets.  Returns their number or a negative error (the
 * reference's sentence in afq_host_last_error()).  Out, each optional and holding `cap` elements: entry[i] ascending, target[i] (the
 * canonical barcode; 0 for a deferred entry), kind[i] (0 exact source, 1 structurally unique neighbour, 2 deferred: structurally
 * ambiguous under frequency).  *barcode_len and *n_samples receive the list's barcode length and its number of canonical samples. */
int64_t afq_gpl_multi_routing(const uint8_t* text, size_t n, int reverse, uint32_t sample_correction, uint32_t sample_neighborhood, uint64_t* entry,
                              uint64_t* target, uint8_t* kind, size_t cap, uint32_t* barcode_len, uint32_t* n_samples);
/* The argument checks of afq_gpl_multi_hist_rad that precede device work: widths, expected_ori, entries ascending and distinct
 * (AFQ_ERR_INVALID_ARG), fitting b0_bytes (AFQ_ERR_BAD_INPUT), at most 2^31 of them (AFQ_ERR_UNSUPPORTED).  0 when they pass. */
int afq_gpl_multi_check_args(uint32_t b0_bytes, uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, const uint64_t* sample_observed, uint64_t n_entries);

/* The options of `alevin-fry convert` (src/main.rs, bam2rad of src/convert.rs:167-594). */
struct afq_convert_stats;
typedef struct afq_convert_opts {
    const char* bam;            /* -b : the input; must end in .bam or .BAM (SAM text is not read)                          */
    const char* rad_out;        /* -o : the RAD file to write; its parent directory is created, an existing file replaced  */
    uint32_t num_threads;       /* -t : BGZF blocks are inflated on max(1, num_threads - 1) threads (convert.rs:205-210)   */
    uint32_t filter_best;       /* -f : keep only the alignments of a read whose AS equals the read's best                 */
    uint32_t device;
    struct afq_convert_stats* stats_out;   /* optional */
} afq_convert_opts;
/* Runs the whole `convert` sub-command in ONE device fill: the BGZF container is inflated on the host - or, through afq_convert_with
 * below, on the device - (every block's CRC32 and ISIZE verified; an empty block mid-file and a missing EOF marker are accepted), the BAM header read, the lengths of CR / UR of the
 * file's first record taken for cblen / ulen, the records handed to afq_convert_bam_rad (include/afquant.h has the record semantics
 * and their errors), and the prelude (convert.rs:238-370) and chunks written only after the device call succeeded.
 * AFQ_ERR_UNSUPPORTED: a path ending in .sam / .SAM.  AFQ_ERR_BAD_INPUT: any other ending ("unsupported input file format, must end
 * with bam/BAM or sam/SAM"), a file that cannot be opened, "BGZF block <i>: ..." for a truncated block, a bad gzip magic, a bad CRC
 * or ISIZE, a bad BAM header, a file without records, a first record without CR / UR, with one that is not of type Z, or of length
 * 0 or above 32, "record <i>: ..." for a block_size that runs past the stream; also an output file that cannot be created or
 * written ("could not write ..."): the library has no code for I/O failures, and its other writers report theirs the same way. */
int afq_convert(const afq_convert_opts* opts);
/* afq_convert with flags: afq_convert(o) is afq_convert_with(o, 0); unknown flag bits are AFQ_ERR_INVALID_ARG.
 * AFQ_CONVERT_INFLATE_ON_DEVICE (`convert --inflate-on-device`): the BGZF blocks are inflated on the device
 * (afq_bgzf_inflate_device of include/afquant.h) and the inflated bytes never cross from host to device.  The host plans the
 * blocks, inflates only the leading ones with zlib until the BAM header is whole, and has the device lay the file down so that
 * the first record stands at a 16-byte-aligned address; the record stream comes back once, for the first record's lengths and
 * the span table, and afq_convert_bam_rad runs on the resident stream.  The RAD file, the stats and the stderr lines are
 * afq_convert's, except that the line about decompression threads says that the device inflates; a bad block is named with
 * afq_convert's words where they do not come from zlib ("bad CRC32", "ISIZE says ..."), otherwise with "the deflate stream is
 * corrupt or longer than ISIZE (<what the device's parser found>)". */
#define AFQ_CONVERT_INFLATE_ON_DEVICE 1u
int afq_convert_with(const afq_convert_opts* opts, uint32_t flags);
/* The prelude afq_convert writes in front of the chunks (convert.rs:238-370): is_paired = 0, the reference names, num_chunks, the
 * file tags cblen:u16 and ulen:u16, the read tags b and u (1, 2, 4 or 8 bytes for lengths 1-4, 5-8, 9-16, 17-32), the alignment
 * tag compressed_ori_refid:u32, the two values.  Returns its length (out may be NULL), or a negative AFQ_ERR_ code.  For tests:
 * it lets the prelude be compared without a device. */
int64_t afq_convert_prelude_bytes(const char* const* ref_names, uint64_t n_ref, uint64_t num_chunks, uint32_t cblen, uint32_t ulen, uint8_t* out, size_t cap);
/* `alevin-fry view` (src/convert.rs:596-709): the records of a RAD file with read tags b and u as text, one line per alignment,
 * `ID:{id}\tHI:{i+1}\tNH:{n}\tCB:{bases}\tUMI:{bases}\tDIR:{true|false}\t{ref name}`, behind the lines `i:name` of the references when
 * print_header is set.  out_path NULL writes to stdout.  AFQ_ERR_UNSUPPORTED: a b or u tag that is not an integer of 1-8 bytes.
 * AFQ_ERR_BAD_INPUT: a missing b / u / cblen / ulen tag, chunks that do not tile the file, a reference id that names no reference. */
int afq_view_file(const char* rad, int print_header, const char* out_path);

/* Runs the whole `quant` sub-command.  Returns 0 or a negative AFQ_ERR_* code; message via afq_host_last_error(). */
int afq_quantify(const afq_quant_opts* opts);
const char* afq_host_last_error(void);

/* ---- pieces exposed for the CPU tests (no GPU needed) ---- */
/* Rust `{}` formatting of an f32 (shortest round-trip digits, never an exponent; "NaN", "inf"). Returns length. */
int afq_format_f32(float v, char* buf, size_t cap);
/* Snappy *frame format* decode (what `snap::read::FrameDecoder` undoes, src/quant.rs:376). out may be NULL to size. */
int64_t afq_snappy_frame_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap);
/* correction_plan.bin (src/correction_plan.rs: magic "AFCORR\0\0", u16 version 1, bincode of CorrectionPlan) and the legacy
 * permit_map.bin (bincode HashMap<u64, u64>).  Each returns the number of corrections of the global cell scope, or a negative
 * error with its reason in afq_host_last_error(): truncated file, bad magic, wrong version, trailing data, a sample-scoped
 * plan.  observed / corrected may both be NULL to size; otherwise they hold `cap` entries and at most `cap` are written.
 * cell_barcode_len (may be NULL) receives the plan's barcode length. */
int64_t afq_parse_correction_plan(const uint8_t* in, size_t n, uint64_t* observed, uint64_t* corrected, size_t cap, uint32_t* cell_barcode_len);
int64_t afq_parse_permit_map(const uint8_t* in, size_t n, uint64_t* observed, uint64_t* corrected, size_t cap);
/* A SAMPLE-SCOPED correction_plan.bin (what afq_generate_permit_list_multi writes): the sample corrections (at most sample_cap
 * written, *n_sample their number), per cell scope that names a sample its canonical sample barcode and the number of its
 * corrections (scope_cap, *n_scopes), and the scopes' corrections back to back in scope order (cell_cap).  Returns their total
 * number, or afq_parse_correction_plan's errors; a plan that is NOT sample-scoped is refused.  Every output may be NULL. */
int64_t afq_parse_correction_plan_multi(const uint8_t* in, size_t n, uint64_t* sample_observed, uint64_t* sample_corrected, size_t sample_cap, uint64_t* n_sample,
                                        uint64_t* scope_barcode, uint64_t* scope_count, size_t scope_cap, uint64_t* n_scopes, uint64_t* cell_observed,
                                        uint64_t* cell_corrected, size_t cell_cap, uint32_t* sample_barcode_len, uint32_t* cell_barcode_len);
/* Parse a RAD prelude; fills the scalars, returns the byte offset of the first chunk or a negative error. */
typedef struct afq_rad_info {
    uint64_t ref_count, num_chunks, first_chunk_off;
    uint32_t is_paired, cblen, ulen, bc_bytes, umi_bytes;
} afq_rad_info;
int afq_rad_parse_prelude(const uint8_t* bytes, size_t n, afq_rad_info* out);

#ifdef __cplusplus
}
#endif
#endif
