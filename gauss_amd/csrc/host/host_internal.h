// libgauss_host.so -- what its translation units share: the data model of the reference's feeder (src/snp.h:14-110,
// src/gauss.h:18-99), result tables, the arena a window's SNP map lives in, the cached file images, and the prototypes of
// the routines that cross files.  Nothing here is exported: the library is built with -fvisibility=hidden and only the C ABI
// of include/gauss_host.h is visible.
//   host_feeder.cpp   the reference's readers and filters (ReadInputZ, ReadReferenceIndex, MakeSnpVec, ReadAnnotation, ...), the
//                     packed-panel cache and open_panel, prepare()
//   host_tables.cpp   result tables, the JEPEG k x k tail, the table accessors of the C ABI
//   host_calls.cpp    the one-window / one-call entry points (computeLD, dist, distmix, qcat, prep_*, jepeg, jepegmix)
//   host_riders.cpp   what a one-window call asks beyond its plain table: leave-one-out, signal selection (+ cond), many traits (+ miss)
//   host_popwgt.cpp   afmix / cpw2: study allele frequencies against the panel's, per-interval weights on the GPU
//   host_chrom.cpp    resident panels, the chromosome driver's own window, gauss_host_impute_chromosome / _genome
#pragma once
#pragma GCC visibility push(default)
#include "../../../include/gauss_host.h"
#pragma GCC visibility pop

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <sstream>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/file.h>
#include <fcntl.h>
#include <unistd.h>
#include <cerrno>

#include <mutex>

#include "bgzf_io.h"
#include "packed_panel.h"

using gauss_host::BgzfReader;
using gauss_host::PackedPanel;
using gauss_host::PkSnp;

// ------------------------------------------------------------------------------------------
extern thread_local std::string g_err;          // host_tables.cpp; gauss_host_last_error() returns it
int herr(const char* fmt, ...);

// Diagnostics on stderr: GAUSS_TRACE=chrom,prep (any subset, or "all"; libgauss_hip reads job, upload, stream from the same variable)
inline bool host_trace(const char* what)
{
    const char* e = getenv("GAUSS_TRACE");
    return e && *e && (strstr(e, "all") != nullptr || strstr(e, what) != nullptr);
}

// ------------------------------------------------------------------------------------------
// tables
// ------------------------------------------------------------------------------------------
struct Column {
    std::string name;
    int type;
    std::vector<std::string> s;
    mutable std::string joined;      // lazily built NUL-separated image of s (gauss_table_strcol)
    mutable std::vector<char> fixed; // lazily built fixed-width image of s (gauss_table_strcol_fixed)
    mutable int fixed_w = 0;
    std::vector<int32_t> i;
    std::vector<double> d;
};

void build_fixed_image(const Column& col);      // Column::fixed / fixed_w (host_tables.cpp)

struct NamedMat {
    std::string name;
    int nrow = 0, ncol = 0;
    std::vector<double> d;        // column-major (R NumericMatrix layout)
};

struct gauss_table {
    std::vector<Column> cols;
    std::vector<double> matrix;
    int matrix_n = 0;
    std::vector<NamedMat> named;
    std::vector<std::string> messages;   // per-window failure texts of a chromosome run
    int nrow() const
    {
        if (cols.empty()) return 0;
        const Column& c = cols[0];
        return (int)(c.type == GAUSS_COL_STR ? c.s.size() : c.type == GAUSS_COL_INT ? c.i.size() : c.d.size());
    }
    // room for MAX_COLS columns (the widest table, dist_cond's 15) is reserved on first use, so the reference add() returns stays
    // valid while the caller adds the columns that follow; one column more than that would move them all, so it is refused.
    // A builder that appends to a finished table (cs_output: dist_cond's 15 and three more) asks for its room with widen()
    // BEFORE its first add(), while it holds no reference into the table
    enum { MAX_COLS = 16 };
    size_t room = MAX_COLS;
    void widen(size_t more) { room = std::max(room, cols.size() + more); cols.reserve(room); }
    Column& add(const char* name, int type)
    {
        if (cols.size() >= room) throw std::length_error("gauss_table::add: no room for another column (MAX_COLS, or what widen() asked for)");
        cols.reserve(room); Column c; c.name = name; c.type = type; cols.push_back(std::move(c)); return cols.back();
    }
    // a named matrix from column-major data (NamedMat's own layout), taken over without a copy
    void put_named(const char* name, int nrow, int ncol, std::vector<double> colmajor)
    {
        NamedMat nm;
        nm.name = name; nm.nrow = nrow; nm.ncol = ncol; nm.d = std::move(colmajor);
        named.push_back(std::move(nm));
    }
};

// ------------------------------------------------------------------------------------------
// data model (src/snp.h:14-110, src/gauss.h:18-99)
// ------------------------------------------------------------------------------------------
struct Snp {
    std::string rsid = ".";
    int chr = -1;
    long long bp = -1;
    std::string a1 = ".", a2 = ".";
    double af1mix = -1.0, af1ref = -1.0;
    double af1study = -1.0;        // afmix / cpw2: the study's allele frequency (Snp::af1study_, ReadInputAf gauss.cpp:211-262)
    double z = 0.0, info = -1.0;
    int qcat_m = 0;                // snp.cpp:26-28
    double qcat_t = 0.0, qcat_chisq = 0.0;
    int type = -1;                 // 0 panel only, 1 GWAS and panel, 2 GWAS only (snp.h:61)
    long long fpos = -1;
    std::string geneid = ".";
    std::map<int, double> categ;   // Snp::categ_map_
    bool flip_geno = false;        // UpdateSnpToMinorAllele (gauss.cpp:1137-1184): genotype d -> 2 - d
    std::string line;              // cached panel data line (read once instead of twice)
    bool have_line = false;
    std::vector<std::pair<const char*, int>> geno;   // selected populations' genotype strings (into `line`)
};

struct MapKey {
    int chr; long long bp; std::string a1, a2;
    bool operator<(const MapKey& r) const     // gauss.h:77-91
    {
        if (chr == r.chr) {
            if (bp == r.bp) {
                if (a1 == r.a1) return a2 < r.a2;
                return a1 < r.a1;
            }
            return bp < r.bp;
        }
        return chr < r.chr;
    }
};
// A window's SNP map lives in blocks of its own instead of the C library's heap.  A 100 000-SNP chromosome enters ~126 000 Snp
// objects and as many map nodes (~480 B a SNP, ~60 MB over the 36 windows); on the FIRST call of a process every page of that is
// touched for the first time -- ~14 000 minor faults, 40 ms of kernel time next to 50 ms of user time for the whole data layer,
// spread over the worker threads' fresh malloc arenas (measured, docs/HISTORY.md section 9e item 9).  Blocks are 2 MB, 2 MB-aligned,
// advised as huge pages and populated in one call (one fault or one batched population instead of 512 traps); a window frees
// nothing one by one -- its blocks go back to a process-wide list when the window is closed, so later calls touch no new page.
struct BlockPool {
    std::mutex mu;
    std::vector<void*> idle;
    size_t keep;
    size_t block;
    BlockPool(size_t block_bytes, size_t keep_bytes) : keep(keep_bytes / block_bytes), block(block_bytes) {}
    void* get()
    {
        {
            std::lock_guard<std::mutex> lock(mu);
            if (!idle.empty()) { void* b = idle.back(); idle.pop_back(); return b; }
        }
        char* raw = (char*)mmap(nullptr, 2 * block, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (raw == (char*)MAP_FAILED) throw std::bad_alloc();
        char* b = (char*)(((uintptr_t)raw + block - 1) & ~(uintptr_t)(block - 1));
        if (b > raw) munmap(raw, (size_t)(b - raw));
        if (b + block < raw + 2 * block) munmap(b + block, (size_t)(raw + 2 * block - (b + block)));
#ifdef MADV_HUGEPAGE
        if (block >= ((size_t)2 << 20)) madvise(b, block, MADV_HUGEPAGE);   // advice only: without huge pages the block is 512 small ones
#endif
#ifdef MADV_POPULATE_WRITE
        madvise(b, block, MADV_POPULATE_WRITE);                         // Linux 5.14+; an older kernel faults the pages in on first use
#endif
        return b;
    }
    void put(void* b)
    {
        {
            std::lock_guard<std::mutex> lock(mu);
            if (idle.size() < keep) { idle.push_back(b); return; }
        }
        munmap(b, block);
    }
};
// Two sizes: a window's FIRST block is small (128 KB: a fine-grained run -- thousands of windows of a few hundred SNPs -- must not
// hold 2 MB apiece), everything after it comes in 2 MB blocks.  GAUSS_HOST_ARENA_KEEP_MB: idle memory kept for the next call
// (default 256 MB in large blocks + 32 MB in small ones); GAUSS_HOST_ARENA_BLOCK_KB (tests): the large block's size, so that a
// small window spans several.  Never destroyed: windows may outlive static destructors.
struct BlockPools {
    BlockPool* small_;
    BlockPool* large_;
    BlockPools()
    {
        size_t large = (size_t)2 << 20;
        if (const char* b = getenv("GAUSS_HOST_ARENA_BLOCK_KB")) {
            size_t kb = 64;
            while (kb < (size_t)std::max(64, atoi(b)) && kb < 2048) kb *= 2;
            large = kb << 10;
        }
        const char* e = getenv("GAUSS_HOST_ARENA_KEEP_MB");
        const size_t keep = (size_t)(e ? std::max(0, atoi(e)) : 256) << 20;
        large_ = new BlockPool(large, keep);
        small_ = new BlockPool(std::min<size_t>(large, (size_t)128 << 10), keep / 8);
    }
};
BlockPools& block_pools();      // host_feeder.cpp (one per process, never destroyed)

struct Arena {
    std::vector<std::pair<void*, BlockPool*>> blocks;
    std::vector<void*> big;
    char* cur = nullptr;
    size_t left = 0;
    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    void* alloc(size_t n)
    {
        n = (n + 15) & ~(size_t)15;
        if (n > left) {
            BlockPools& bp = block_pools();
            BlockPool* from = blocks.empty() ? bp.small_ : bp.large_;
            if (n > from->block / 8) { void* q = ::operator new(n); big.push_back(q); return q; }
            cur = (char*)from->get();
            blocks.emplace_back(cur, from);
            left = from->block;
        }
        void* q = cur;
        cur += n; left -= n;
        return q;
    }
    ~Arena()
    {
        for (auto& b : blocks) b.second->put(b.first);
        for (void* q : big) ::operator delete(q);
    }
};

template <class T>
struct ArenaAlloc {
    typedef T value_type;
    Arena* a;
    explicit ArenaAlloc(Arena* arena) : a(arena) {}
    template <class U> ArenaAlloc(const ArenaAlloc<U>& o) : a(o.a) {}
    T* allocate(size_t n) { return (T*)a->alloc(n * sizeof(T)); }
    void deallocate(T*, size_t) {}                                      // the blocks go back as a whole
    template <class U> bool operator==(const ArenaAlloc<U>& o) const { return a == o.a; }
    template <class U> bool operator!=(const ArenaAlloc<U>& o) const { return a != o.a; }
};

struct SnpDestroy { void operator()(Snp* s) const { s->~Snp(); } };     // storage is the arena's
typedef std::unique_ptr<Snp, SnpDestroy> SnpPtr;
struct SnpMapArena { Arena arena; };
typedef std::map<MapKey, SnpPtr, std::less<MapKey>, ArenaAlloc<std::pair<const MapKey, SnpPtr>>> SnpMapBase;
struct SnpMap : private SnpMapArena, public SnpMapBase {               // the arena is built before the map and outlives it
    SnpMap() : SnpMapBase(std::less<MapKey>(), ArenaAlloc<std::pair<const MapKey, SnpPtr>>(&arena)) {}
    SnpMap(const SnpMap&) = delete;
    SnpMap& operator=(const SnpMap&) = delete;
    SnpPtr make() { return SnpPtr(new (arena.alloc(sizeof(Snp))) Snp()); }
};

struct Args {                       // Arguments, gauss.h:18-69 with the defaults of gauss.cpp:18-35
    int chr = 0;
    long long start_bp = 0, end_bp = 0, wing_size = 0;
    std::string study_pop, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, annotation_file;
    std::vector<std::string> ref_pop_vec, ref_sup_pop_vec;
    std::vector<int> ref_pop_size_vec;
    double lambda = 0.1, min_abs_eig = 1e-5, eig_cutoff = 0.01;
    std::vector<int> pop_flag_vec;
    std::vector<double> pop_wgt_vec;
    std::map<std::string, double> pop_wgt_map;
    int num_pops = 0, num_samples = 0;
    double af1_cutoff = 0.01;
    int min_num_measured_snp = 10, min_num_unmeasured_snp = 10;
    std::shared_ptr<PackedPanel> pk;   // set when reference_data_file is a packed panel (packed_panel.h)
    // dist / distmix on a packed panel: a panel SNP that no study SNP shares its position with and that lies in a wing
    // would enter the map as type 0 (gauss.cpp:373-385), pass the AF filter and then be dropped by the partition
    // (dist.cpp:132-140 imputes type-0 SNPs of the prediction window only; the output is cut to it, dist.cpp:91-93) --
    // nothing ever reads it, so it is not entered at all (about half of an extended window's panel SNPs)
    bool drop_wing_unmeasured = false;
    // jepeg / jepegmix drivers: only study SNPs at positions the annotation names (and the study's odd positions, above) enter the SNP
    // map -- every step after ReadInputZ touches entries of ONE position at a time, the gene table is made of annotated SNPs alone,
    // and a chromosome's study is four times the annotated SNPs (host_calls.cpp:run_jepeg; GAUSS_HOST_FULL_MAP=1: the whole study)
    bool annotated_only = false;
    int total_num_categ = 6;
    double categ_cor_cutoff = 0.8;
    int denorm_norm_w = 3;
};

// whitespace tokeniser with the semantics of `istringstream >> a >> b ...` for well-formed lines
struct Tok {
    const char* p; const char* e;
    explicit Tok(const std::string& s) : p(s.data()), e(s.data() + s.size()) {}
    // whitespace as std::isspace in the "C" locale (what operator>> skips), from a table: panel lines are ~33 kB
    // of genotype digits and this scan runs over every byte of them
    static const bool* ws_table()
    {
        static const struct T { bool t[256]; T() { for (int c = 0; c < 256; c++) t[c] = (c == ' ' || (c >= 9 && c <= 13)); } } tab;
        return tab.t;
    }
    bool next(const char*& b, int& n)
    {
        const bool* ws = ws_table();
        while (p < e && ws[(unsigned char)*p]) p++;
        if (p >= e) return false;
        b = p;
        // long tokens (a population's genotype string) end at a blank in practice: let memchr find it, then
        // make sure no other white-space character came first
        const char* q = (const char*)memchr(p, ' ', (size_t)(e - p));
        const char* lim = q ? q : e;
        const char* r = p;
        while (r < lim && !ws[(unsigned char)*r]) {
            // skip ahead in blocks of 8 digits while there is room
            if (lim - r >= 8 && !(ws[(unsigned char)r[0]] | ws[(unsigned char)r[1]] | ws[(unsigned char)r[2]] | ws[(unsigned char)r[3]] |
                                  ws[(unsigned char)r[4]] | ws[(unsigned char)r[5]] | ws[(unsigned char)r[6]] | ws[(unsigned char)r[7]])) r += 8;
            else r++;
        }
        p = r;
        n = (int)(p - b);
        return true;
    }
    bool str(std::string& out) { const char* b; int n; if (!next(b, n)) return false; out.assign(b, n); return true; }
    bool i64(long long& out) { std::string t; if (!str(t)) return false; char* q; out = strtoll(t.c_str(), &q, 10); return q != t.c_str(); }
    bool i32(int& out) { long long v; if (!i64(v)) return false; out = (int)v; return true; }
    bool dbl(double& out) { std::string t; if (!str(t)) return false; char* q; out = strtod(t.c_str(), &q); return q != t.c_str(); }
};


// Parsed image of a GWAS summary file (rsid chr bp a1 a2 z), kept per process and shared by every window of a
// chromosome run that names the same file (path + size + mtime): the reference re-reads the text once per call
// (gauss.cpp:146-152).  Rows are in file order and carry the reference's parsing-state semantics: a field that
// fails to parse keeps the value of the previous line (the variables live outside the loop there too).
struct GwasRow { std::string rsid, a1, a2; int chr; long long bp; double z; };
struct GwasCache {
    std::vector<GwasRow> rows;
    std::vector<uint32_t> by_pos;      // row numbers ordered by (chr, bp), file order among equals: a window takes its range by binary search
    // positions the study lists more than once, or under equal alleles: the only ones where the reference's duplicate check
    // (gauss.cpp:386-392) can fire -- the gene drivers keep them in their SNP map whatever the annotation names (sorted)
    std::vector<std::pair<int, long long>> odd_positions;
};

// ------------------------------------------------------------------------------------------
// prepared window / gene set
// ------------------------------------------------------------------------------------------
struct gauss_prepared {
    int kind = 0;
    Args args;
    SnpMap snp_map;
    std::vector<Snp*> snp_vec;                 // after the AF filter, map order
    std::vector<Snp*> measured, unmeasured;    // matrix row order
    std::vector<int32_t> measured_rows, unmeasured_rows;
    std::vector<uint8_t> gm, gu;
    int64_t ld = 0;
    int N = 0;
    std::vector<int32_t> pop_off;
    std::vector<double> pop_wgt, z1;
    std::vector<int32_t> gene_off;
    std::vector<double> out_z, out_info, out_r, out_b11, out_b21;
    int n_head = 0, n_predm = 0;               // QCAT: measured SNPs left of / inside the prediction window
    // packed panel: rows stay in the mmap'd file and are named by index (zero-copy); gm / gu are only
    // materialised (as ASCII) for the kinds that need bytes on the host
    bool packed_rows = false;
    std::vector<int32_t> store_rows_m, store_rows_u, pop_src_off;
    int32_t num_eig = 0;
    int32_t status = 0;
    gauss_table snps;
    bool snps_built = false;
};

struct GeneResult {
    std::string geneid = ".", top_categ = ".", top_snp = ".";
    double chisq = -1.0, jepeg_pval = -1.0, top_categ_pval = -1.0, top_snp_pval = -1.0;
    int df = 0, num_snp = 0;
};

// minimal fork-join helper: fn(i) for i in [0, n) on up to nt threads
template <typename F>
inline void parallel_for(int n, int nt, F fn)
{
    if (n <= 0) return;
    nt = std::max(1, std::min(nt, n));
    if (nt == 1) { for (int i = 0; i < n; i++) fn(i); return; }
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    auto body = [&]() { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i); };
    for (int t = 1; t < nt; t++) th.emplace_back(body);
    body();
    for (std::thread& x : th) x.join();
}

inline bool env_flag(const char* name, bool dflt)
{
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the chromosome driver's window (host_chrom.cpp: a merge of the sorted study and panel tables); also behind the one-window
// entry points of host_calls.cpp ----
struct ChromSetup {                     // what prepare() derives from a call's arguments alone: once per call, not once per window
    int kind = 0;
    bool mix = false, qcat = false;
    bool measured_only = false;         // computeLD: unmeasured SNPs are never read (computeLD.cpp:80-86) -- not entered at all
    bool lds = false;                   // LD scores: every panel SNP of the extended window is entered; the targets are the study's SNPs inside it
    Args a;                             // population table, flags, weights, cutoffs (start_bp / end_bp are the windows', not set here)
    std::vector<int> sel;               // the selected populations, panel order
    std::vector<int32_t> pop_off, pop_src_off;
    std::vector<double> pop_wgt;
    double two_subj = 0;                // 2 x the selected samples (gauss.cpp:589)
    std::shared_ptr<const GwasCache> gw;
};

struct LeanSnp {
    int64_t row;                        // panel row = fpos of the packed feeder
    long long bp;
    double z, info, af;
    int32_t type, qcat_m;
    double qcat_t, qcat_chisq;
};

struct LeanWindow {
    const ChromSetup* cs = nullptr;
    long long start_bp = 0, end_bp = 0;
    std::vector<LeanSnp> v;             // prepare()'s snp_vec: after the AF filter, map order
    std::vector<int32_t> measured, unmeasured;      // into v, matrix row order
    std::vector<int32_t> store_rows_m, store_rows_u;
    std::vector<double> z1, out_z, out_info, out_r;
    int n_head = 0, n_predm = 0;
    int32_t num_eig = 0, status = 0;
    std::unique_ptr<gauss_table> pre;   // the output table, built while the GPU works (lean_table_prebuild); the results are filled in after
    std::vector<int32_t> out_row;       // v -> row of the table, -1 outside the prediction window
    // the chromosome driver builds no table per window: the window's rows are a slice [tab_off, tab_off + n_out) of the call's ONE table
    size_t tab_off = 0;
    int n_out = -1;                     // rows of the prediction window (lean_table_count)
    // A window handed out by the window cache owns none of the lists above: `base` is the cached (immutable) window they are read
    // from -- lean_src() -- and this object holds the call's own state only (outputs, status, its slice of the table).  The chromosome
    // driver's functions (lean_window_desc, lean_table_count, lean_table_prebuild_into, lean_window_finish_into) read through lean_src.
    std::shared_ptr<const LeanWindow> base;
};
static inline const LeanWindow& lean_src(const LeanWindow& w) { return w.base ? *w.base : w; }
// The slice form of lean_table_prebuild / lean_window_finish: the window's rows written straight into the columns of `all` (which must
// hold the reference's column set, sized to cover the slice) -- everything the results do not change before the GPU is waited for,
// the unmeasured SNPs' z / info / pval (QCAT: the four test columns) after.  Slices of different windows may be written concurrently.
int lean_table_count(LeanWindow& w);
void lean_table_prebuild_into(LeanWindow& w, gauss_table& all, size_t off);
void lean_window_finish_into(LeanWindow& w, gauss_table& all);
// A pristine copy of a built window (the inputs; nothing a call writes) -- what the window cache keeps and hands out
std::unique_ptr<LeanWindow> lean_window_clone(const LeanWindow& w);

int chrom_setup(ChromSetup& cs, int kind, int chr, int64_t wing_size, const char* study_pop, const char* const* pop_names,
                const double* pop_wgts, int n_pop_wgt, const char* input_file, const std::string& packed_path, const char* desc_file,
                double af1_cutoff, const std::shared_ptr<PackedPanel>& pk, const std::shared_ptr<const GwasCache>& gw);
int lean_window_build(LeanWindow& w, const ChromSetup& cs, long long start_bp, long long end_bp);
int lean_window_desc(LeanWindow& w, gauss_window_desc* d);
void lean_table_prebuild(LeanWindow& w);
gauss_table* lean_window_finish(LeanWindow& w);

// The columns every SNP table opens with -- rsid chr bp a1 a2 -- for rows 0 .. n - 1, each described by at(i): a Snp of the SNP
// map, or a row of the packed panel's SNP table (LeanSnp::bp is that row's position).  The caller adds its own columns after.
struct SnpIdent { const char* rsid; int chr; long long bp; const char* a1; const char* a2; };
inline SnpIdent ident_of(const Snp& s) { return {s.rsid.c_str(), s.chr, s.bp, s.a1.c_str(), s.a2.c_str()}; }
inline SnpIdent ident_of(const PackedPanel& pk, const LeanSnp& sn)
{
    const PkSnp& ps = pk.snp(sn.row);
    return {pk.str(ps.rsid), ps.chr, sn.bp, pk.str(ps.a1), pk.str(ps.a2)};
}
template <class F>
inline void add_ident_columns(gauss_table& t, size_t n, F at)
{
    Column &rsid = t.add("rsid", GAUSS_COL_STR), &chr = t.add("chr", GAUSS_COL_INT), &bp = t.add("bp", GAUSS_COL_INT);
    Column &a1 = t.add("a1", GAUSS_COL_STR), &a2 = t.add("a2", GAUSS_COL_STR);
    for (Column* c : {&rsid, &a1, &a2}) c->s.reserve(n);
    for (Column* c : {&chr, &bp}) c->i.reserve(n);
    for (size_t i = 0; i < n; i++) {
        const SnpIdent s = at(i);
        rsid.s.emplace_back(s.rsid); chr.i.push_back(s.chr); bp.i.push_back((int)s.bp);
        a1.s.emplace_back(s.a1); a2.s.emplace_back(s.a2);
    }
}
inline void add_ident_columns(gauss_table& t, const std::vector<Snp*>& rows) { add_ident_columns(t, rows.size(), [&](size_t i) { return ident_of(*rows[i]); }); }

// ---- routines that cross translation units ----
int read_ref_desc(Args& a);
int init_pop_flag_vec(Args& a);
void init_pop_flag_wgt_vec(Args& a);
void set_pop_wgt_map(Args& a, const char* const* names, const double* w, int n);
std::shared_ptr<const GwasCache> load_gwas_cached(const std::string& path, std::string& err);
int ReadInputZ(SnpMap& m, const Args& a, bool All);
int ReadInputAf(SnpMap& m, const Args& a);
int host_threads();
int merge_index_entry(SnpMap& m, const Args& a, bool All, const std::string& rsid, int chr, long long bp,
                             const std::string& a1, const std::string& a2, long long fpos);
int ReadReferenceIndex(SnpMap& m, const Args& a, bool All);
void load_line(BgzfReader& fp, Snp& s, const Args& a, std::vector<double>* af_out);
std::shared_ptr<PackedPanel> open_packed_shared(const std::string& path, std::string& err);
// the panel of a call: its packed form from the cache where GAUSS_AUTO_PACK allows, opened when packed (host_feeder.cpp)
int open_panel(const char* index_file, const std::string& data_file, const char* desc_file, std::string& path,
               std::shared_ptr<PackedPanel>& pk, bool require_packed = false);
int open_panel_all_pops(Args& a, const char* index_file);
int panel_matches_desc(const Args& a, const PackedPanel& pk, bool names);
std::vector<int32_t> panel_pop_off(const Args& a, int* N);
int files_ok(std::initializer_list<const char*> names);       // "file name is NULL"
void fill_matrix(std::vector<uint8_t>& G, const std::vector<Snp*>& rows, int64_t ld);
void unpack_rows(const gauss_prepared& p, const std::vector<Snp*>& rows, std::vector<uint8_t>& G);
void materialise_from_packed(gauss_prepared& p);
void build_snp_table(gauss_prepared& p);
int prepare(gauss_prepared& p);
double pnorm_upper(double x);
double pchisq_upper(double x, int df);
GeneResult jepeg_tail(const std::vector<Snp*>& gs, const double* CorG, const Args& a);
gauss_table* dist_output(gauss_prepared& p);
gauss_table* qcat_output(gauss_prepared& p);
// dist_loo / distmix_loo: one row per measured SNP of the prediction window, `idx` its row among the window's measured SNPs (the
// index into the three leave-one-out arrays of gauss_window_desc)
struct LooRow { SnpIdent id; double af, z; int idx; };
gauss_table* loo_output(bool mix, const std::vector<LooRow>& rows, const double* loo_z, const double* loo_info, const double* loo_t);
// One SNP of a window as the tables and the riders read it, whichever way the window was built (host_calls.cpp: CallWindow).  The
// strings of `id` point into the window: a ViewSnp does not outlive it.
struct ViewSnp { SnpIdent id; double af, z; int wing; };     // af: af1mix | af1ref; wing: 0 inside [start_bp, end_bp] (dist.cpp:92), else 1
using SlctRow = ViewSnp;                                      // the names the stand-alone programs of the host tests build their rows under
using LdsRow = ViewSnp;                                       // (id and af; ldscore_output reads no more)
// dist_slct / distmix_slct: one row per measured SNP of the EXTENDED window, matrix row order (row i = index i of the selection's arrays)
gauss_table* slct_output(bool mix, const std::vector<ViewSnp>& rows, int n_sel, const int32_t* idx, const double* zin, const double* joint,
                         const double* zc, const double* var_left);
// dist_cond / distmix_cond: dist_output's table `t` of the same call, the measured SNPs of the wings appended (rows = every measured
// SNP of the extended window as for slct_output; row_m[i] / row_u[i] = the table row of measured / unmeasured SNP i, -1 when the
// table does not list it), the columns wing order z_cond pval_cond var_left added -- imputed rows carry cond_z / cond_var -- and the
// named matrix `signals` [n_sel x 3]: table row (from 0), z_entry, z_joint.  -1 (message set, `t` untouched) when `t` has a column
// that is not one of dist_output's
int cond_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                 int n_sel, const int32_t* idx, const double* zin, const double* joint, const double* zc, const double* var_left,
                 const double* cond_z, const double* cond_var);
// dist_cs / distmix_cs: cond_output's table `t` of the same call (its `at` rows: every measured SNP has one), the columns pip cs
// cs_pip added -- cs = the 1-based order of entry of the credible set that holds the SNP (the `order` column's numbering), 0 for none
// -- and the named matrix `sets` [n_sel x 4]: table row of the lead SNP (from 0), size, mass, lse.  pip / set / set_pip are indexed by
// candidate: the M = rows.size() measured SNPs first, then the unmeasured ones.  -1 (message set) when `t` is not cond_output's
int cs_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
              int n_sel, const int32_t* idx, const double* pip, const int32_t* set, const double* set_pip,
              const int32_t* size, const double* mass, const double* lse);
// dist_susie / distmix_susie: the call's own table `t` with the wings' measured SNPs appended (cond_output's rows) and the columns wing
// pip cs cs_pip added -- cs = the 1-based effect of the kept set that holds the SNP, 0 for none -- the named matrices `effects` [L x 7]
// (table row of the SNP of largest alpha from 0, V, lse, size, mass, purity, kept) and `fit` [1 x 3] (sweeps, delta, converged), and a
// message when the sweeps ran out or the window was not fitted.  pip / set / set_pip / alpha [L][T] are indexed by candidate
int susie_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                 int L, double tol, const double* pip, const int32_t* set, const double* set_pip, const double* alpha, const double* V,
                 const double* lse, const int32_t* size, const double* mass, const double* purity, const int32_t* kept, const double* sweeps);
// dist_xsusie / distmix_xsusie, the joint fit across studies.  xs_build_map: plain arrays in, plain array out -- key_lead [n_lead] and
// key_peer [n_peer] name the panel SNP every candidate of the leader and of a peer is (any 64-bit key that is equal for the same SNP);
// from_lead [n_lead] gets the peer's candidate index of leader candidate j, -1 where the peer has no such SNP (gauss_window_desc.
// xs_from_lead).  Returns the number of shared candidates, or -1 (herr) when a study names one SNP twice.
int xs_build_map(const int64_t* key_lead, size_t n_lead, const int64_t* key_peer, size_t n_peer, int32_t* from_lead);
// ... and the table: `t` is study 1's susie_output table (the joint pip / cs / cs_pip in its rows); adds the column `joint` (1: the SNP
// is a candidate of every study; joint [M + U] by leader candidate, row_m / row_u as susie_output takes them), replaces the named
// matrix `effects` by [L x (2 K + 5)]: table row of the SNP of largest alpha, V_1 .. V_K, purity_1 .. purity_K, lse, size, mass, kept
// (xs_V / xs_purity [K][L]; the others are columns of susie_output's `effects`), and says which study kept the group from being
// fitted (status [K]: the windows' GAUSS_ST_* bits)
int xsusie_output(gauss_table& t, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u, const uint8_t* joint, int K, int L,
                  const double* xs_V, const double* xs_purity, const int32_t* status);
// dist_coloc / distmix_coloc: susie_output's rows and its columns wing pip cs cs_pip for trait 1, then pip_t cs_t cs_pip_t for every
// further fitted trait t = 2 .. 1 + k; traits_output's named matrices over ALL rows (a wing's measured SNP shows its own study z); the
// named matrices effects_t and fit_t (susie_output's `effects` and `fit`) for t = 1 .. 1 + k; and `coloc`, one row per pair of kept
// effects of two traits: trait_a trait_b (1-based) cs_a cs_b (the 1-based effects, the cs / cs_t columns' numbering) n H0 H1 H2 H3 H4
// hit_row (table row of the most likely shared SNP, from 0) hit_pp.  A message per trait whose sweeps ran out or that was not fitted
struct SusieFit {                     // one trait's out_susie_* (first) or the further traits' out_coloc_more_* with a leading [k] (more)
    const double *pip, *set_pip, *alpha, *V, *lse, *mass, *purity, *sweeps;
    const int32_t *set, *size, *kept;
};
struct ColocMore { int k; SusieFit fit; const double* pp; const int32_t* hit; const double* hit_pp; const int32_t* n; };
int coloc_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                 int L, double tol, const SusieFit& first, int n_more, const double* z_more, const double* out_z_more, const ColocMore& more);
// dist_ldscore / distmix_ldscore: a table of its own, one row per target: rsid chr bp a1 a2 af1ref|af1mix l2 l2_raw n_band, and the named
// matrix `ldscore` [1 x 4]: n_eff, M (reference rows of the window, targets included), M_5_50 (those with min(af, 1 - af) > 0.05), radius
// (rows: id and af are read)
gauss_table* ldscore_output(bool mix, const std::vector<ViewSnp>& rows, const double* l2, const double* raw, const double* mass, double n_eff,
                            int64_t n_ref, int64_t n_ref_5_50, int64_t radius);
// Kish's effective size of a weighted panel: (sum w_p)^2 / sum (w_p^2 / n_p) over the populations of non-zero weight; sizes [P]
double kish_n_eff(const double* w, const int32_t* pop_off, int P);
// dist_prs / distmix_prs: a table of its own, one row per measured SNP of the extended window: rsid chr bp a1 a2 af1ref|af1mix z r wing
// (r = z / sqrt(n - 2 + z^2), 0 where z is not finite: such a SNP is frozen at weight 0), the named matrices `beta` [n_s n_lam x rows],
// grid cell i_s n_lam + i_lam, and `grid` [n_s n_lam x 9]: s, lam, nnz, sweeps, delta, br, bg, kkt, converged; a message when a cell
// ran its sweeps out and when the window was not fitted.  beta [n_s][n_lam][rows]
gauss_table* prs_output(bool mix, const std::vector<ViewSnp>& rows, double n, double tol, const std::vector<double>& s,
                        const std::vector<double>& lam, const double* beta, const int32_t* nnz, const int32_t* sweeps, const double* delta,
                        const double* br, const double* bg, const double* kkt);
// dist_traits / distmix_traits: the Z-scores of one further trait at the n measured SNPs of a window.  SNP i is at(i) -- position and
// alleles in the window's (the panel's) orientation -- and is looked up in the study `gw` (read from `path`, named in the messages)
// by (chr, bp, a1, a2): the same allele order gives z, the swapped order -z (gauss.cpp:358-370); of several rows that match, the
// later one wins; rows for other SNPs are ignored.  Refused: a SNP without a row (the message names the file, the first missing
// rsid and how many are missing) and a z that is not finite.
// With miss_out [n] (dist_traits_miss / distmix_traits_miss): a SNP without a row sets miss_out[i] = 1 (z_out[i] = 0) instead of being
// refused, and *n_missing counts them; a z that is present and not finite is still refused.
int traits_match(const GwasCache& gw, const char* path, size_t n, const std::function<SnpIdent(size_t)>& at, double* z_out,
                 uint8_t* miss_out = nullptr, size_t* n_missing = nullptr);
// The limits of a window whose further files lack SNPs, checked before any GPU work; mask [n_more][M] as traits_match filled it, paths
// [n_more] name the files in the messages.  Refused, naming the file, the count and the limit: a file that lacks more than
// GAUSS_TRAITS_MISS_MAX of the window's measured SNPs, one left with min_measured or fewer (the reference would refuse that trait:
// dist.cpp:145-151), and a window in which more than GAUSS_TRAITS_MISS_UNION_MAX distinct SNPs are missing.
int traits_miss_limits(const char* const* paths, int n_more, size_t M, const uint8_t* mask, int min_measured);
// what the window returned for the SNPs the further traits lack (miss_more / out_info_more / out_z_miss / out_info_miss of gauss_window_desc)
struct TraitsMiss { const uint8_t* mask; const double* info_more; const double* z_miss; const double* info_miss; };
// ... and their part of the table: `t` is dist_output's table of trait 1, unchanged; two named matrices are added, z_traits and
// pval_traits [nrow x (1 + n_more)], column 0 the table's own z / pval, column 1 + k trait k: for a measured SNP its own study z
// (z_more [n_more][M]), for an unmeasured one the imputed z (out_z_more [n_more][U]); pval = 2 pnorm(-|z|).  row_m[i] / row_u[i]:
// the table row of measured / unmeasured SNP i, -1 when the table does not list it (the wings)
// With `miss` (the *_traits_miss calls): info_traits and type_traits [nrow x (1 + n_more)] are added, column 0 the table's own info /
// type; a measured SNP that trait k lacks shows its imputed z, its info and type 0 in column 1 + k, an unmeasured SNP the trait's own
// info; and n_missing [1 + n_more]: how many of the window's measured SNPs (wings included) each trait's file lacked (trait 1: 0).
void traits_output(gauss_table& t, int n_more, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                   const double* z_more, const double* out_z_more, const TraitsMiss* miss = nullptr);
// the smallest chi^2 (1 df) whose two-sided p-value 2 pnorm_upper(sqrt(chi2)) is below p, to the bit
double slct_chi2_of(double p);

// ---- the riders of a one-window call (host_riders.cpp; run by host_calls.cpp:run_impute) ----
// What a rider reads of the window of its call, filled once by the window itself (host_calls.cpp: CallWindow::view -- the lean window
// on a sorted packed panel, or gauss_prepared).  It points into the window: a view does not outlive it.
struct WindowView {
    bool mix = false;
    std::vector<ViewSnp> measured;                  // the measured SNPs of the EXTENDED window, matrix row order
    std::vector<int32_t> row_m, row_u;              // row of the call's own table for measured / unmeasured SNP i, -1: not listed (the wings)
    std::function<int(gauss_table**)> plain;        // the call's own table: dist_output / lean_window_finish
};
// A rider: what a call asks of its window beyond the plain table.  A call has at most one.  It owns the buffers the window writes.
//   check()  the refusals that need no window (before the panel is opened)
//   ask()    sizes the buffers, sets its fields of the descriptor, refuses what the window shows to be wrong
//   table()  the call's table from the view and the filled buffers
struct Rider {
    virtual ~Rider() = default;
    virtual int check() { return 0; }
    virtual int ask(gauss_window_desc& d, const WindowView& v) = 0;
    virtual int table(const WindowView& v, gauss_table** out) = 0;
};
// dist_loo / distmix_loo: the three leave-one-out arrays of gauss_window_desc; the table lists the measured SNPs of the prediction
// window (the wings only contribute to B11)
struct LooRider : Rider {
    std::vector<double> z, info, t;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};
// dist_slct / distmix_slct: the slct_* fields; the table lists every measured SNP of the extended window (a signal in a wing must be
// conditioned on, not hidden).  unmeasured (dist_cond / distmix_cond): the imputed SNPs conditioned on the selection too -- the
// call's own table with the selection's columns added (cond_output)
struct SlctRider : Rider {
    double p_cutoff, collin; int max_signals; const char* const* cond; int n_cond; bool unmeasured;      // the call's own arguments
    SlctRider(double p_cutoff_, double collin_, int max_signals_, const char* const* cond_, int n_cond_, bool unmeasured_)
        : p_cutoff(p_cutoff_), collin(collin_), max_signals(max_signals_), cond(cond_), n_cond(n_cond_), unmeasured(unmeasured_) {}
    int32_t n = 0;
    std::vector<int32_t> idx, forced;
    std::vector<double> zin, joint, zc, var, cond_z, cond_var;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};
// dist_traits / distmix_traits: the call's input file is trait 1 and defines the window exactly as in the plain call; every further
// file is matched to the window's measured SNPs (traits_match) and rides in the same single job as n_traits_more / z_more; the table
// is the plain call's with the named matrices of traits_output added.  miss (the *_traits_miss calls): a measured SNP a further
// file lacks becomes a bit of miss_more instead of an error, and the window returns that trait's own info and the imputed z of the
// SNPs it lacks (traits_miss_limits: the limits, before any GPU work)
// dist_cs / distmix_cs: dist_cond's rider (window, selection and conditional columns are built once, by SlctRider with unmeasured set)
// with the cs_* fields of gauss_window_desc; the table is dist_cond's with the columns and the named matrix of cs_output added
struct CsRider : SlctRider {
    double coverage, prior_var;                                        // the call's own arguments; <= 0 or NaN: 0.95 / 25.0
    CsRider(double p_cutoff_, double collin_, int max_signals_, const char* const* cond_, int n_cond_, double coverage_, double prior_var_)
        : SlctRider(p_cutoff_, collin_, max_signals_, cond_, n_cond_, true), coverage(coverage_), prior_var(prior_var_) {}
    std::vector<double> pip, set_pip, mass, lse;
    std::vector<int32_t> set, size;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};
// dist_susie / distmix_susie: the susie_* fields of gauss_window_desc; the table is the call's own with every measured SNP of the
// extended window listed (susie_output).  Independent of the selection
struct SusieRider : Rider {
    int L, max_sweeps, estimate_prior_var, measured_only;              // the call's own arguments; <= 0 or NaN: the defaults (ask)
    double coverage, prior_var, min_abs_corr, tol;
    SusieRider(int L_, double coverage_, double prior_var_, double min_abs_corr_, int max_sweeps_, double tol_, int estimate_prior_var_,
               int measured_only_)
        : L(L_), max_sweeps(max_sweeps_), estimate_prior_var(estimate_prior_var_), measured_only(measured_only_), coverage(coverage_),
          prior_var(prior_var_), min_abs_corr(min_abs_corr_), tol(tol_) {}
    int n_eff = 0;
    double tol_used = 0.0;
    std::vector<double> pip, set_pip, alpha, V, lse, mass, purity, sweeps;
    std::vector<int32_t> set, size, kept;
    int check() override;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};
// dist_prs / distmix_prs: the prs_* fields of gauss_window_desc; the table lists every measured SNP of the extended window with its
// weights over the grid (prs_output).  Independent of the selection
struct PrsRider : Rider {
    double n, tol; int max_sweeps;                                     // the call's own arguments; tol 0 or NaN, max_sweeps <= 0: the defaults (ask)
    std::vector<double> s, lam;                                        // the grid; an empty list: lassosum's (the constructor)
    int n_s_arg, n_lam_arg;
    PrsRider(double n_, const double* s_, int n_s, const double* lam_, int n_lam, double tol_, int max_sweeps_);
    double tol_used = 0.0;
    std::vector<double> beta, delta, br, bg, kkt;
    std::vector<int32_t> nnz, sweeps;
    int check() override;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};
struct TraitsRider : Rider {
    const char* const* files; int n_more; bool miss;                   // the call's own arguments: the further files
    TraitsRider(const char* const* files_, int n_more_, bool miss_) : files(files_), n_more(n_more_), miss(miss_) {}
    std::vector<double> z, out_z, info, z_miss, info_miss;
    std::vector<uint8_t> mask;
    int check() override;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};
// dist_coloc / distmix_coloc: TraitsRider's files and matching (no mask: a further file that lacks a measured SNP is refused) and
// SusieRider's arguments in one window; every further trait is fitted beside trait 1 (coloc_traits_more = n_more) and every pair of
// fitted traits is colocalised (coloc_p1 / coloc_p2 / coloc_p12; <= 0 or NaN: coloc's 1e-4, 1e-4, 1e-5).  The table is coloc_output's
struct ColocRider : Rider {
    TraitsRider traits;
    SusieRider susie;
    double p1, p2, p12;
    ColocRider(const char* const* files_, int n_more_, const SusieRider& susie_, double p1_, double p2_, double p12_)
        : traits(files_, n_more_, false), susie(susie_), p1(p1_), p2(p2_), p12(p12_) {}
    std::vector<double> pip, set_pip, alpha, V, lse, mass, purity, sweeps, pp, hit_pp;      // the further traits [k][..], the pairs
    std::vector<int32_t> set, size, kept, hit, n;
    int check() override;
    int ask(gauss_window_desc& d, const WindowView& v) override;
    int table(const WindowView& v, gauss_table** out) override;
};

gauss_table* prep_output(gauss_prepared& p);
int panel_make_resident(gauss_ctx* ctx, const std::string& path, void** dev, int64_t* uploaded, bool async = false);
bool panel_is_resident(gauss_ctx* ctx, const std::string& path, void** dev, bool wait = true);
// zmix's SNP selection, shared by prep_zmix5, the prep_zmix selectors and zmix (host_calls.cpp)
struct ZmixStudy { Args a; SnpMap m; std::vector<Snp*> measured; };       // the panel, the merged SNP map, its type-1 SNPs in map order
int zmix_read(ZmixStudy& st, const char* input_file, const char* reference_index_file, const char* reference_data_file,
              const char* reference_pop_desc_file);
int zmix_ai_select(ZmixStudy& st, int step, double pct, std::vector<int>& kept, std::vector<double>& kept_nv, std::vector<Snp*>* sel);
int zmix_genotypes(Args& a, const std::vector<Snp*>& sel, int N, int64_t* ld, std::vector<uint8_t>& G);
int zmix_sup_groups(const Args& a, std::vector<int32_t>& pop_group, std::vector<std::string>& names);
// computeLD's measured SNPs and where their genotype rows are (host_calls.cpp), shared by computeLD and simulateLD
struct LdRows {
    std::unique_ptr<gauss_table> t;     // the snplist columns: rsid chr bp a1 a2 af1mix
    std::vector<double> z;              // [M] the study's Z-scores of the rows (computeLD and simulateLD do not read them; clump does)
    int M = 0;
    const uint8_t* store = nullptr;     // rows as gauss_ld_rows takes them
    int64_t ld = 0;
    int geno_fmt = GAUSS_GENO_U8, on_device = 0;
    std::vector<int32_t> rows;          // store rows (empty: rows 0 .. M - 1)
    std::vector<int32_t> pop_off, pop_src_off;      // selected populations, panel order (pop_src_off empty for U8 rows)
    std::vector<double> pop_wgt;
    Args a;                             // population table, flags and weight map of the call
    std::shared_ptr<PackedPanel> pk;    // what keeps `store` alive
    std::unique_ptr<gauss_prepared> prep;
    // the source as a C entry point takes it: NULL for "rows 0 .. M - 1" and for "no source offsets"
    const int32_t* row_ptr() const { return rows.empty() ? nullptr : rows.data(); }
    const int32_t* src_off_ptr() const { return pop_src_off.empty() ? nullptr : pop_src_off.data(); }
    int n_pop() const { return (int)pop_off.size() - 1; }
};
int computeld_rows(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                   int n_pop_wgt, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                   const char* reference_pop_desc_file, double af1_cutoff, LdRows& out);
// clump(): the thresholds of gauss_ld_clump_rows for key = z^2 from the call's p-values and distances (host_tables.cpp).  NaN (not
// given) takes PLINK's value: p1 1e-4, p2 1e-2, r2 0.5, kb 250; key = slct_chi2_of(p), so a SNP is an index iff its two-sided p-value is
// below p1.  -1 with the message set: p1 or p2 outside (0, 1], p2 < p1, r2 outside [0, 1], kb < 0 or not finite
struct ClumpKeys { double key_index, key_member, r2_min; int64_t radius; };
int clump_keys(double p1, double p2, double r2, double kb, ClumpKeys& out);
// ... and its table: `t` holds computeLD's snplist columns (rsid chr bp a1 a2 af1mix); z pval clump index_rsid r2 are added -- pval =
// 2 pnorm(-|z|), clump = the rank of the SNP's clump (0: none), index_rsid = the lead's rsid ("." for none), r2 = the squared LD to
// it -- and the named matrix `clumps` [n_clumps x 4], one row per clump in rank order: index row (from 0), size, bp of the first
// member, bp of the last.  owner / rank / r2 [M] as gauss_ld_clump_rows returned them
void clump_output(gauss_table& t, const std::vector<double>& z, const int32_t* owner, const int32_t* rank, const double* r2, int n_clumps);
// ldsplit(): the arguments of gauss_ld_split_rows from the call's (host_tables.cpp).  NaN / 0 (not given) takes the default: thr_r2 0.02,
// min_size 50, max_size 1000, max_K GAUSS_LDSPLIT_MAX_K, max_r2 0.3, kb none (the band is max_size alone).  -1 with the message set:
// thr_r2 or max_r2 outside [0, 1], a size or max_K outside gauss_ld_split_rows' limits, min_size > max_size, kb < 0 or not finite
struct LdSplitParams { double thr_r2, max_r2; int min_size, max_size, max_K; int64_t radius; };
int ldsplit_params(double thr_r2, int min_size, int max_size, int max_K, double max_r2, double kb, LdSplitParams& out);
// ... and its table: `t` holds computeLD's snplist columns and keeps them; four named matrices are added -- `splits` [n x 5], one row
// per K that has a split, ascending: n_block, cost, perc_kept (sum of size^2 / M^2), cost2 (sum of size^2), max_size_used; `last`
// [n x the largest such K]: the table row of every block's last SNP, -1 beyond the row's K; `max_r2_at` [M + 1 x 1]: Mx; `n_nonfinite`
// [1 x 1].  cost [max_K], prev [max_K][M + 1], mx [M + 1] as gauss_ld_split_rows returned them; the splits are read backwards from prev
void ldsplit_output(gauss_table& t, int M, int max_K, const double* cost, const int32_t* prev, const double* mx, int64_t n_nonfinite);
// hess(): its table (host_tables.cpp): `t` holds computeLD's snplist columns and keeps them; four named matrices are added -- `z`
// [M x T], the traits' Z-scores at the SNPs (file k in column k, signs as the first file's alleles); `lam` [M x 1]; `proj` [T x k_max];
// `solve` [1 x 4]: n_pos, sweeps, n_nonfinite, status.  z [T][M], lam [M], proj [T][k_max] as gauss_ld_hess_rows took and returned them
void hess_output(gauss_table& t, int M, int T, int k_max, const double* z, const double* lam, const double* proj, int n_pos, int sweeps,
                 int64_t n_nonfinite, int status);
// sumchi2(): P(sum lambda_i chi2_1 > q) (host_tables.cpp; the method: gauss_host_sumchi2_pval in include/gauss_host.h).  lambda_i <= 0
// or NaN are left out; n_pos (may be null): how many stay
double sumchi2_pval(const double* lam, int n, double q, int* n_pos);
// ... and its table, one row per gene: geneid num_snp num_kept chisq pval lam_max n_pos status top_snp top_snp_pval message, and the
// named matrix `lam` [n_gene x 128].  gene_off [n_gene + 1] into rsid / z (the measured list); n_kept, q, top, status [n_gene] and lam
// [n_gene][128] as gauss_gene_sumchi2 returned them for one trait (null with n_gene = 0)
gauss_table* sumchi2_output(const std::vector<std::string>& geneid, const std::vector<int32_t>& gene_off, const std::vector<std::string>& rsid,
                            const std::vector<double>& z, const int32_t* n_kept, const double* lam, const double* q, const int32_t* top,
                            const int32_t* status);
