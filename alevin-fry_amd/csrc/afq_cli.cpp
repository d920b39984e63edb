// afq_cli.cpp — `afquant quant …`, `afquant infer …`, `afquant generate-permit-list …`, `afquant collate …`, `afquant convert …`, `afquant view …`, `afquant atac collate …`: the flag surfaces of `alevin-fry quant` (src/main.rs:294-348 of the
// reference) and `alevin-fry infer` (src/main.rs:350-365) in front of afq_quantify() / afq_infer_files()
// (include/afquant_host.h).  Same spellings and defaults; what the reference refuses (--use-eds, -b with a plain
// resolution, -d with trivial, --summary-stat without -b) is refused here too, with its message.
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/afquant.h"
#include "../../include/afquant_host.h"

static void usage() {
    std::fprintf(stderr,
                 "usage: afquant quant -i <input-dir> -m <tg-map> -o <output-dir> -r <resolution>\n"
                 "       [-t <threads>] [--small-thresh N] [--umi-edit-dist 0|1] [--large-graph-thresh N]\n"
                 "       [--quant-subset FILE] [--init-uniform] [--use-mtx] [-d] [-b N] [--device N | --devices 0,1,...]\n"
                 "       [--summary-stat] [--boot-seed S] [--sa-model winner-take-all|prefer-ambig] [--sz-on-device]\n"
                 "resolutions: trivial cr-like cr-like-em parsimony parsimony-em parsimony-gene parsimony-gene-em\n"
                 "       afquant atac deduplicate -i <input-dir> [-t N] [-d fw|rc] [--device N] [--sz-on-device]\n"
                 "       afquant atac sort -i <input-dir> -r <rad-dir> [-t N] [-c] [-m N] [--device N]\n"
                 "       afquant atac collate -i <input-dir> -r <rad-dir> [-t N] [-c] [-m N] [--device N]   (-m is without effect; -c is not supported)\n"
                 "       afquant generate-permit-list -i <input-dir> -d fw|rc|both|either -o <output-dir> (-k | -e N | -f N | -b FILE | -u FILE [-m MINREADS])\n"
                 "       [-t N] [--cell-bc-correction unique|frequency] [--cell-bc-neighborhood hamming-1|substitution-or-shift-1|edit-1]\n"
                 "       [--cell-bc-confidence 0.975|a/b] [--device N] [--fill-bytes BYTES]\n"
                 "       afquant collate -i <input-dir> -r <rad-dir> [-t N] [--device N]   (one device fill: -m/--max-records, --memory-limit and\n"
                 "       --collation-mode are accepted and without effect; -c/--compress is not supported)\n"
                 "       afquant convert -b <file.bam> -o <out.rad> [-t N] [-f] [--device N] [--inflate-on-device]   (-f/--filter_best: only a read's best-AS alignments; SAM text is not read;\n"
                 "       --inflate-on-device: the BGZF blocks are inflated on the device instead of on -t host threads)\n"
                 "       afquant view -r <file.rad> [-H]   (one line per alignment on stdout; -H/--header: the reference names first)\n"
                 "       afquant infer -c <geqc_counts.mtx> -e <gene_eqclass.txt.gz> -o <output-dir> [--usa] [--quant-subset FILE] [-t N]\n");
}

int main(int argc, char** argv) {
    // The rows of a range come back over PCIe while the next range's kernels run: that copy belongs on the DMA engines.  Left to
    // itself the HIP runtime moves some of these copies with blit kernels on the compute queue, where they take a millisecond of
    // the next decode (profiles/r04_timeline_*.txt); this keeps every copy on SDMA.  Read by the runtime at its first call.
    setenv("GPU_FORCE_BLIT_COPY_SIZE", "0", 0);
    if (argc >= 2 && (std::strcmp(argv[1], "-h") == 0 || std::strcmp(argv[1], "--help") == 0)) { usage(); return 0; }
    if (argc >= 2 && (std::strcmp(argv[1], "-V") == 0 || std::strcmp(argv[1], "--version") == 0)) {
        std::printf("afquant-hip 0.1 (alevin-fry 0.18.0 quant / infer semantics, C ABI version %d)\n", AFQ_ABI_VERSION);
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "infer") == 0) {   // src/main.rs:350-365, 825-847
        afq_infer_opts io{};
        auto need2 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-c" || a == "--count-mat") io.count_mat = need2(i);
            else if (a == "-e" || a == "--eq-labels") io.eq_labels = need2(i);
            else if (a == "-o" || a == "--output-dir") io.output_dir = need2(i);
            else if (a == "-t" || a == "--threads") io.num_threads = (uint32_t)std::atoi(need2(i));
            else if (a == "--usa") io.usa_mode = 1;
            else if (a == "--quant-subset") io.filter_list = need2(i);
            else if (a == "--use-mtx") {}
            else if (a == "--use-eds") { std::fprintf(stderr, "--use-eds is no longer supported. EDS output has been removed as of v0.12.\n"); return 1; }
            else if (a == "--device") io.device = (uint32_t)std::atoi(need2(i));
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!io.count_mat || !io.eq_labels || !io.output_dir) { usage(); return 2; }
        const int rc = afq_infer_files(&io);
        if (rc) { std::fprintf(stderr, "afquant infer failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "atac") == 0 && std::strcmp(argv[2], "generate-permit-list") == 0) {
        std::fprintf(stderr, "afquant: `atac generate-permit-list` is not supported; only `generate-permit-list` for single-barcode RNA RAD files is\n");
        return 1;
    }
    if (argc >= 2 && std::strcmp(argv[1], "generate-permit-list") == 0) {   // src/main.rs:170-269, 392-577
        afq_gpl_opts go{};
        go.min_reads = 10; go.neighborhood = -1; go.conf_num = 39; go.conf_den = 40;
        std::string cmdline;
        for (int i = 0; i < argc; ++i) { if (i) cmdline += ' '; cmdline += argv[i]; }
        go.cmdline = cmdline.c_str();
        int n_methods = 0;
        bool have_ori = false;
        auto need2 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        auto count_arg = [&](int& i, const char* flag, uint64_t& v) -> bool {
            const char* t = need2(i);
            char* e = nullptr;
            errno = 0;
            v = std::strtoull(t, &e, 10);
            if (e == t || *e || errno || t[0] == '-') { std::fprintf(stderr, "error: invalid value '%s' for '%s': invalid digit found in string\n", t, flag); return false; }
            return true;
        };
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-i" || a == "--input") go.input_dir = need2(i);
            else if (a == "-o" || a == "--output-dir") go.output_dir = need2(i);
            else if (a == "-d" || a == "--expected-ori") {
                std::string v = need2(i);
                for (auto& ch : v) ch = (char)std::toupper((unsigned char)ch);
                if (v == "FW") go.expected_ori = 1; else if (v == "RC") go.expected_ori = 2; else if (v == "BOTH" || v == "EITHER") go.expected_ori = 0;
                else { std::fprintf(stderr, "error: invalid value '%s' for '--expected-ori <EXPECTEDORI>'\n  [possible values: fw, rc, both, either]\n", argv[i]); return 2; }
                have_ori = true;
            }
            else if (a == "-k" || a == "--knee-distance") { go.method = AFQ_GPL_KNEE; ++n_methods; }
            else if (a == "-e" || a == "--expect-cells") { go.method = AFQ_GPL_EXPECT; ++n_methods; if (!count_arg(i, "--expect-cells <EXPECTCELLS>", go.method_count)) return 2; }
            else if (a == "-f" || a == "--force-cells") { go.method = AFQ_GPL_FORCE; ++n_methods; if (!count_arg(i, "--force-cells <FORCECELLS>", go.method_count)) return 2; }
            else if (a == "-b" || a == "--valid-bc") { go.method = AFQ_GPL_VALID_BC; ++n_methods; go.list_file = need2(i); }
            else if (a == "-u" || a == "--unfiltered-pl") { go.method = AFQ_GPL_UNFILTERED; ++n_methods; go.list_file = need2(i); }
            else if (a == "-m" || a == "--min-reads") { if (!count_arg(i, "--min-reads <MINREADS>", go.min_reads)) return 2; }
            else if (a == "-t" || a == "--threads") go.num_threads = (uint32_t)std::atoi(need2(i));
            else if (a == "--cell-bc-correction") {
                const std::string v = need2(i);
                if (v == "unique") go.frequency = 0; else if (v == "frequency") go.frequency = 1;
                else { std::fprintf(stderr, "error: invalid value '%s' for '--cell-bc-correction <STRATEGY>'\n  [possible values: unique, frequency]\n", v.c_str()); return 2; }
            }
            else if (a == "--cell-bc-neighborhood") {
                const std::string v = need2(i);
                if (v == "hamming-1") go.neighborhood = 0; else if (v == "substitution-or-shift-1" || v == "edit-1") go.neighborhood = 1;
                else { std::fprintf(stderr, "error: invalid value '%s' for '--cell-bc-neighborhood <NEIGHBORHOOD>'\n  [possible values: hamming-1, substitution-or-shift-1, edit-1]\n", v.c_str()); return 2; }
            }
            else if (a == "--cell-bc-confidence") {
                const char* v = need2(i);
                if (afq_gpl_parse_confidence(v, &go.conf_num, &go.conf_den)) { std::fprintf(stderr, "error: invalid value '%s' for '--cell-bc-confidence <CONFIDENCE>': %s\n", v, afq_host_last_error()); return 2; }
            }
            else if (a == "--memory-limit" || a == "--tmp-dir") (void)need2(i);   // accepted and ignored: they size the reference's deferred sample buffers
            else if (a.rfind("--sample-", 0) == 0) {
                std::fprintf(stderr, "afquant generate-permit-list: %s is not supported: multi-barcode (--sample-bc-list) input is not supported\n", a.c_str());
                return 1;
            }
            else if (a == "--device") go.device = (uint32_t)std::atoi(need2(i));
            else if (a == "--fill-bytes") { if (!count_arg(i, "--fill-bytes <BYTES>", go.fill_bytes)) return 2; }   // chunk bytes per device fill (default 8 GiB)
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!go.input_dir || !go.output_dir || !have_ori) {
            std::fprintf(stderr, "error: the following required arguments were not provided:\n%s%s%s", go.input_dir ? "" : "  --input <INPUT>\n", have_ori ? "" : "  --expected-ori <EXPECTEDORI>\n",
                         go.output_dir ? "" : "  --output-dir <OUTPUTDIR>\n");
            usage();
            return 2;
        }
        if (n_methods != 1) {
            std::fprintf(stderr, n_methods ? "error: the filter methods --knee-distance, --expect-cells, --force-cells, --valid-bc and --unfiltered-pl cannot be used with one another\n"
                                           : "error: the following required arguments were not provided:\n  <--knee-distance|--expect-cells <EXPECTCELLS>|--force-cells <FORCECELLS>|--valid-bc <VALIDBC>|--unfiltered-pl <UNFILTEREDPL>>\n");
            usage();
            return 2;
        }
        if (go.method == AFQ_GPL_UNFILTERED && go.min_reads < 1) { std::fprintf(stderr, "min-reads < 1 is not supported, the value %llu was provided\n", (unsigned long long)go.min_reads); return 1; }
        if (go.num_threads < 2) go.num_threads = 2;   // (minimum: 2; lower values use 2)
        uint64_t corrected = 0;
        go.corrected_out = &corrected;
        const int rc = afq_generate_permit_list(&go);
        if (rc) { std::fprintf(stderr, "afquant generate-permit-list failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        if (corrected == 0) std::fprintf(stderr, "found 0 corrected barcodes; please check the input.\n");
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "collate") == 0) {   // src/main.rs:271-292, 579-610
        afq_collate_opts co{};
        co.max_records = 30000000;
        std::string cmdline;
        for (int i = 0; i < argc; ++i) { if (i) cmdline += ' '; cmdline += argv[i]; }
        co.cmdline = cmdline.c_str();
        auto need2 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-h" || a == "--help") { usage(); return 0; }
            else if (a == "-i" || a == "--input-dir") co.input_dir = need2(i);
            else if (a == "-r" || a == "--rad-dir") co.rad_dir = need2(i);
            else if (a == "-t" || a == "--threads") co.num_threads = (uint32_t)std::atoi(need2(i));
            else if (a == "-c" || a == "--compress") co.compress = 1;
            else if (a == "-m" || a == "--max-records") co.max_records = (uint32_t)std::strtoul(need2(i), nullptr, 10);   // one device fill: without effect
            else if (a == "--memory-limit" || a == "--collation-mode") (void)need2(i);                                   // ... as are these
            else if (a == "--device") co.device = (uint32_t)std::atoi(need2(i));
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!co.input_dir || !co.rad_dir) {
            std::fprintf(stderr, "error: the following required arguments were not provided:\n%s%s", co.input_dir ? "" : "  --input-dir <INPUTDIR>\n", co.rad_dir ? "" : "  --rad-dir <RADDIR>\n");
            usage();
            return 2;
        }
        for (const char* flag : {"-i", "-r"}) {   // clap's pathbuf_directory_exists_validator (main.rs:276-281)
            const char* dir = flag[1] == 'i' ? co.input_dir : co.rad_dir;
            FILE* probe = std::fopen(dir, "r");
            if (!probe) { std::fprintf(stderr, "error: invalid value '%s' for '%s': the directory does not exist\n", dir, flag[1] == 'i' ? "--input-dir <INPUTDIR>" : "--rad-dir <RADDIR>"); return 2; }
            std::fclose(probe);
        }
        const int rc = afq_collate(&co);
        if (rc) { std::fprintf(stderr, "afquant collate failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "convert") == 0) {   // bam2rad, src/convert.rs:167-594
        afq_convert_opts vo{};
        vo.num_threads = 8;
        uint32_t vflags = 0;
        auto need2 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-h" || a == "--help") { usage(); return 0; }
            else if (a == "-b" || a == "--bam") vo.bam = need2(i);
            else if (a == "-o" || a == "--output") vo.rad_out = need2(i);
            else if (a == "-t" || a == "--threads") vo.num_threads = (uint32_t)std::atoi(need2(i));
            else if (a == "-f" || a == "--filter_best") vo.filter_best = 1;
            else if (a == "--device") vo.device = (uint32_t)std::atoi(need2(i));
            else if (a == "--inflate-on-device") vflags |= AFQ_CONVERT_INFLATE_ON_DEVICE;
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!vo.bam || !vo.rad_out) {
            std::fprintf(stderr, "error: the following required arguments were not provided:\n%s%s", vo.bam ? "" : "  --bam <BAM>\n", vo.rad_out ? "" : "  --output <OUTPUT>\n");
            usage();
            return 2;
        }
        const int rc = afq_convert_with(&vo, vflags);
        if (rc) { std::fprintf(stderr, "afquant convert failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "view") == 0) {   // src/convert.rs:596-709
        const char* rad = nullptr;
        int header = 0;
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-h" || a == "--help") { usage(); return 0; }
            else if (a == "-r" || a == "--rad") { if (i + 1 >= argc) { usage(); return 2; } rad = argv[++i]; }
            else if (a == "-H" || a == "--header") header = 1;
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!rad) { std::fprintf(stderr, "error: the following required arguments were not provided:\n  --rad <RAD>\n"); usage(); return 2; }
        const int rc = afq_view_file(rad, header, nullptr);
        if (rc) { std::fprintf(stderr, "afquant view failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "atac") == 0 && std::strcmp(argv[2], "collate") == 0) {   // src/main.rs:905-922
        afq_atac_collate_opts co{};
        co.max_records = 30000000;
        std::string cmdline;
        for (int i = 0; i < argc; ++i) { if (i) cmdline += ' '; cmdline += argv[i]; }
        co.cmdline = cmdline.c_str();
        auto need3 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        for (int i = 3; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-h" || a == "--help") { usage(); return 0; }
            else if (a == "-i" || a == "--input-dir") co.input_dir = need3(i);
            else if (a == "-r" || a == "--rad-dir") co.rad_dir = need3(i);
            else if (a == "-t" || a == "--threads") co.num_threads = (uint32_t)std::atoi(need3(i));
            else if (a == "-c" || a == "--compress") co.compress = 1;
            else if (a == "-m" || a == "--max-records") co.max_records = (uint32_t)std::strtoul(need3(i), nullptr, 10);   // one device fill: without effect
            else if (a == "--device") co.device = (uint32_t)std::atoi(need3(i));
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!co.input_dir || !co.rad_dir) {
            std::fprintf(stderr, "error: the following required arguments were not provided:\n%s%s", co.input_dir ? "" : "  --input-dir <INPUTDIR>\n", co.rad_dir ? "" : "  --rad-dir <RADDIR>\n");
            usage();
            return 2;
        }
        for (const char* flag : {"-i", "-r"}) {   // clap's pathbuf_directory_exists_validator (main.rs:907-912)
            const char* dir = flag[1] == 'i' ? co.input_dir : co.rad_dir;
            FILE* probe = std::fopen(dir, "r");
            if (!probe) { std::fprintf(stderr, "error: invalid value '%s' for '%s': the directory does not exist\n", dir, flag[1] == 'i' ? "--input-dir <INPUTDIR>" : "--rad-dir <RADDIR>"); return 2; }
            std::fclose(probe);
        }
        const int rc = afq_atac_collate(&co);
        if (rc) { std::fprintf(stderr, "afquant atac collate failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "atac") == 0 && std::strcmp(argv[2], "deduplicate") == 0) {   // src/main.rs:942-956, atac/run.rs:128-169
        afq_atac_dedup_opts ao{};
        ao.rev = 1;   // --permit-bc-ori defaults to rc
        auto need3 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        for (int i = 3; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-i" || a == "--input-dir") ao.input_dir = need3(i);
            else if (a == "-t" || a == "--threads") ao.num_threads = (uint32_t)std::atoi(need3(i));
            else if (a == "-d" || a == "--permit-bc-ori") {
                std::string v = need3(i);
                for (auto& ch : v) ch = (char)std::toupper((unsigned char)ch);
                if (v == "RC") ao.rev = 1; else if (v == "FW") ao.rev = 0;
                else { std::fprintf(stderr, "invalid barcode orientation %s\n", v.c_str()); return 2; }
            }
            else if (a == "--device") ao.device = (uint32_t)std::atoi(need3(i));
            else if (a == "--sz-on-device") ao.sz_on_device = 1;
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!ao.input_dir) { usage(); return 2; }
        const int rc = afq_atac_deduplicate(&ao);
        if (rc) { std::fprintf(stderr, "afquant atac deduplicate failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "atac") == 0 && std::strcmp(argv[2], "sort") == 0) {   // src/main.rs:924-938
        afq_atac_sort_opts so{};
        so.num_threads = 0; so.max_records = 30000000;   // -t: min(16, cores), at least 2
        std::string cmdline;
        for (int i = 0; i < argc; ++i) { if (i) cmdline += ' '; cmdline += argv[i]; }
        so.cmdline = cmdline.c_str();
        auto need3 = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        for (int i = 3; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-i" || a == "--input-dir") so.input_dir = need3(i);
            else if (a == "-r" || a == "--rad-dir") so.rad_dir = need3(i);
            else if (a == "-t" || a == "--threads") so.num_threads = (uint32_t)std::atoi(need3(i));
            else if (a == "-c" || a == "--compress") so.compress = 1;
            else if (a == "-m" || a == "--max-records") so.max_records = (uint32_t)std::strtoul(need3(i), nullptr, 10);
            else if (a == "--device") so.device = (uint32_t)std::atoi(need3(i));
            else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
        }
        if (!so.input_dir || !so.rad_dir) {
            std::fprintf(stderr, "error: the following required arguments were not provided:\n%s%s", so.input_dir ? "" : "  --input-dir <INPUTDIR>\n", so.rad_dir ? "" : "  --rad-dir <RADDIR>\n");
            usage();
            return 2;
        }
        const int rc = afq_atac_sort(&so);
        if (rc) { std::fprintf(stderr, "afquant atac sort failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
        return 0;
    }
    if (argc < 2 || std::strcmp(argv[1], "quant") != 0) { usage(); return 2; }
    afq_quant_opts o{};
    o.small_thresh = 100; o.umi_edit_dist = -1; o.large_graph_thresh = -1; o.num_threads = 0;
    std::string cmdline;
    std::vector<int32_t> devs;
    for (int i = 0; i < argc; ++i) { if (i) cmdline += ' '; cmdline += argv[i]; }
    o.cmdline = cmdline.c_str();
    auto need = [&](int& i) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-i" || a == "--input-dir") o.input_dir = need(i);
        else if (a == "-m" || a == "--tg-map") o.tg_map = need(i);
        else if (a == "-o" || a == "--output-dir") o.output_dir = need(i);
        else if (a == "-r" || a == "--resolution") o.resolution = need(i);
        else if (a == "-t" || a == "--threads") o.num_threads = (uint32_t)std::atoi(need(i));
        else if (a == "--small-thresh") o.small_thresh = (uint32_t)std::atoi(need(i));
        else if (a == "--umi-edit-dist") o.umi_edit_dist = std::atoi(need(i));
        else if (a == "--large-graph-thresh") o.large_graph_thresh = std::atoi(need(i));
        else if (a == "--quant-subset") o.filter_list = need(i);
        else if (a == "--init-uniform") o.init_uniform = 1;
        else if (a == "--summary-stat") o.summary_stat = 1;
        else if (a == "--boot-seed") o.boot_seed = std::strtoull(need(i), nullptr, 10);
        else if (a == "--use-mtx") {}
        else if (a == "--use-eds") { std::fprintf(stderr, "--use-eds is no longer supported. EDS output has been removed as of v0.12.\n"); return 1; }
        else if (a == "-d" || a == "--dump-eqclasses") o.dump_eq = 1;
        else if (a == "-b" || a == "--num-bootstraps") o.num_bootstraps = (uint32_t)std::atoi(need(i));
        else if (a == "--sa-model") {
            const std::string v = need(i);
            if (v == "winner-take-all") o.sa_model = AFQ_SA_WINNER_TAKE_ALL;
            else if (v == "prefer-ambig") o.sa_model = AFQ_SA_PREFER_AMBIG;
            else { std::fprintf(stderr, "invalid value '%s' for '--sa-model': possible values: prefer-ambig, winner-take-all\n", v.c_str()); return 2; }
        }
        else if (a == "--multi-sample-output") (void)need(i);
        else if (a == "--device") o.device = (uint32_t)std::atoi(need(i));
        else if (a == "--sz-on-device") o.sz_on_device = 1;
        else if (a == "--devices") {   // comma list of HIP device ordinals: cells are range-partitioned over them
            for (const char* p = need(i); *p;) { char* e; const long v = std::strtol(p, &e, 10); if (e == p) { std::fprintf(stderr, "--devices wants a comma list of integers\n"); return 2; } devs.push_back((int32_t)v); p = *e == ',' ? e + 1 : e; if (*e && *e != ',') { std::fprintf(stderr, "--devices wants a comma list of integers\n"); return 2; } }
        }
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (!devs.empty()) { o.devices = devs.data(); o.n_devices = (uint32_t)devs.size(); }
    if (!o.input_dir || !o.tg_map || !o.output_dir || !o.resolution) { usage(); return 2; }
    if ((o.summary_stat || o.init_uniform) && !o.num_bootstraps) {   // clap `requires("num-bootstraps")`, main.rs:306-307
        std::fprintf(stderr, "error: the following required arguments were not provided:\n  --num-bootstraps <NUMBOOTSTRAPS>\n");
        return 2;
    }
    const int rc = afq_quantify(&o);
    if (rc) { std::fprintf(stderr, "afquant quant failed (%d): %s\n", rc, afq_host_last_error()); return 1; }
    // every output file is written and closed: leave without unwinding the HIP runtime and the pinned pools (tens of ms of
    // teardown the operating system does anyway)
    std::fflush(nullptr);
    std::_Exit(0);
}
