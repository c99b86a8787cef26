// gmg_mg_run.h -- the host side of gmg_mg.hip (included at its end: the kernels are static templates of that translation unit).
// gmg_mg_score_reads, gmg_mg_score_groups and gmg_find_orfs run through MgRun: a plan of every path decision (MgPlan, made on
// the host before anything is queued), then one member function per stage.  Every device block of a call belongs to the run's
// GmgScratch; whatever the result does not take goes back to the cache when the run ends.
#ifndef GMG_MG_RUN_H
#define GMG_MG_RUN_H

static unsigned grid_for(uint64_t n);

// gmg_mg_score_groups: consecutive groups of reads, each under its own gene model (NULL / 0: one model for the batch)
struct MgGroups {
    std::vector<const gmg_model *> models;
    std::vector<uint64_t> read_begin;                   // n + 1 entries
    int n = 0;
};

// the gene model's fp32 rows, complete (gmg_launch_gene6_full), for one model or for groups of reads under their own models
static int mg_gene6_full(const gmg_model *gene, const MgGroups *groups, const gmg_reads *reads, float *d_gene32, uint64_t gstride, hipStream_t s)
{
    if (groups && groups->n > 0)
        return gmg_launch_gene6_groups(groups->models.data(), groups->read_begin.data(), groups->n, reads, d_gene32, gstride, s);
    const int rc = gmg_launch_gene6_full(gene, reads, d_gene32, gstride, s);
    if (rc != GMG_EBADMODEL || gene->dev.P < 3) return rc;
    const uint64_t whole[2] = {0, reads->n_reads};      // a model of another shape: the any-shape kernel, as one group
    return gmg_launch_gene6_groups(&gene, whole, 1, reads, d_gene32, gstride, s);
}

// the table of gmg_frame_score6 with read r scored against null model d_read_null[r] (device array, or NULL: model 0)
static int mg_frame6_nulls(const gmg_model *gene, const float *d_null_tab, const uint32_t *d_read_null,
                           const gmg_reads *reads, double *d_out, uint64_t stride, hipStream_t s, const MgGroups *groups = nullptr)
{
    if (reads->total_bases == 0) return GMG_OK;
    const uint64_t gstride = (reads->total_bases + 15) & ~15ull;
    GmgScratch sc(GmgScratch::AFTER, s);
    float *d_gene32 = nullptr;
    GMG_HIP(sc.alloc(&d_gene32, (size_t)6 * gstride * sizeof(float)));
    const int rc = mg_gene6_full(gene, groups, reads, d_gene32, gstride, s);
    if (rc) return gmg_set_error(rc, "per-read null models need a gene model of the default shape (depth 7, window <= 15, periodicity 3)");
    MgArgs a;
    memset(&a, 0, sizeof a);
    a.packed = reads->d_packed;
    a.read_off = reads->d_off;
    a.tile_read = reads->d_tile_read;
    a.n_reads = reads->n_reads;
    a.total = reads->total_bases;
    a.gene32 = d_gene32;
    a.fs_stride = gstride;
    a.null_tab = d_null_tab;
    a.read_null = d_read_null;
    hipLaunchKernelGGL(k_mg_apply_nulls, dim3(grid_for(a.total)), dim3(256), 0, s, a, d_out, stride);
    GMG_HIP(hipGetLastError());
    return GMG_OK;
}

extern "C" int gmg_frame_score6_nulls(const gmg_model *gene, const gmg_null_set *nulls, const uint32_t *read_null,
                                      const gmg_reads *reads, double *d_out, uint64_t row_stride, void *stream)
{
    { int rc_enter = gmg_enter("gmg_frame_score6_nulls"); if (rc_enter) return rc_enter; }
    if (!gene || !nulls || !reads || (!read_null && reads->n_reads) || (!d_out && reads->total_bases))
        return gmg_set_error(GMG_EINVAL, "gmg_frame_score6_nulls: NULL argument");
    if (row_stride < reads->total_bases) return gmg_set_error(GMG_EINVAL, "gmg_frame_score6_nulls: row stride < total_bases");
    if (gene->dev.P < 3) return gmg_set_error(GMG_EBADMODEL, "gmg_frame_score6_nulls: periodicity must be >= 3");
    for (uint64_t r = 0; r < reads->n_reads; r++)
        if (read_null[r] >= (uint32_t)nulls->n)
            return gmg_set_error(GMG_ERANGE, "gmg_frame_score6_nulls: read %llu names null model %u of %d", (unsigned long long)r, read_null[r], nulls->n);
    if (reads->total_bases == 0) return GMG_OK;
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::AFTER, s);
    uint32_t *d_rn = nullptr;
    GMG_HIP(sc.alloc(&d_rn, reads->n_reads * 4));
    GMG_HIP(hipMemcpyAsync(d_rn, read_null, reads->n_reads * 4, hipMemcpyHostToDevice, s));
    GMG_HIP(hipStreamSynchronize(s));                              // (the caller's array may go away when the call returns)
    return mg_frame6_nulls(gene, nulls->d_tab, d_rn, reads, d_out, row_stride, s);
}

static unsigned mg_codon_from(const char *s)            // Codon_t::Set_From (gene.cc:133-146)
{
    unsigned d = 0;
    for (int i = 0; i < 3 && s[i]; i++) d = ((d & 0xffu) << 4) | mg_ch_mask(s[i]);
    return d;
}
static unsigned mg_codon_revcomp(unsigned data)         // Codon_t::Reverse_Complement (gene.cc:96-113)
{
    unsigned x = 0;
    for (int i = 0; i < 12; i++) { x = (x << 1) | (data & 1u); data >>= 1; }
    return x;
}

// scratch and result buffers come from the library's cache of device blocks (gmg_pool_alloc, gmg_api.hip)
static unsigned grid_for(uint64_t n)
{
    const uint64_t blocks = (n + 255) / 256;
    return (unsigned)(blocks < 256 * 16 ? (blocks ? blocks : 1) : 256 * 16);
}

// exclusive sum of cnt[0..n] (cnt[n] = 0) into off[0..n] as 64-bit offsets; *total = off[n]
// d_off[i] = d_cnt[0] + ... + d_cnt[i-1], i <= n, and *total = d_off[n] (synchronises s): one launch (gmg_scan.h)
static int mg_scan(uint32_t *d_cnt, uint64_t *d_off, uint64_t n, uint64_t *total, hipStream_t s)
{
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_cnt, d_off, n + 1, s)));
    GMG_HIP(hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    return GMG_OK;
}

extern "C" int gmg_mg_result_free(gmg_mg_result *r)
{
    if (!r) return GMG_OK;
    delete r;
    return GMG_OK;
}

// GMG_MG_TIMING=1: wall time of every stage on stderr (synchronises after each stage)
struct MgTimer {
    bool on;
    hipStream_t s;
    std::chrono::steady_clock::time_point t0;
    MgTimer(hipStream_t st) : on(gmg_opt(GMG_OPT_MG_TIMING) != 0), s(st), t0(std::chrono::steady_clock::now()) {}
    void lap(const char *what)
    {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[gmg_mg] %-28s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = std::chrono::steady_clock::now();
    }
};

#define MG_RETRY_NO_WAVE 1000    // (internal) the write pass of k_mg_err_wave ran out of stack: the call repeats without the wave kernels
static thread_local int tl_mg_no_wave = 0;
// (what the level passes of this thread's last call handed on per base: a run's chunks are alike, and a count pass that finds its
// arrays too small runs twice -- weakly trained models keep several times the branches of a real one alive)
static thread_local double tl_mg_calls_per_base_hint = 0.0;

static int mg_err_mode(const gmg_mg_params *prm) { return (prm->flags & GMG_MG_ALLOW_INDELS) ? 1 : (prm->flags & GMG_MG_ALLOW_SUBS) ? 2 : 0; }
// Find_Orfs' other two modes (ignore regions, circular sequences): gmg_find_orfs alone -- the start scan of the front half
// indexes Frame_Scores inside one linear read
static bool mg_general(const gmg_mg_params *prm) { return prm->circular != 0 || prm->n_ignore_regions != 0; }

// what a caller may not ask for
static int mg_check_params(const gmg_model *gene, const gmg_model *nul, const gmg_reads *reads, const gmg_mg_params *prm,
                           gmg_mg_result **out, const bool find_only)
{
    if ((!find_only && (!gene || !nul)) || !reads || !prm || !out) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: NULL argument");
    if (prm->n_start_codons < 0 || prm->n_start_codons > 8 || prm->n_stop_codons < 0 || prm->n_stop_codons > 8 ||
        prm->min_gene_len < 4)
        return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: need 0..8 start / stop codons and min_gene_len >= 4");
    if (!find_only && (gene->dev.P != 3 || nul->dev.P != 3))
        return gmg_set_error(GMG_EBADMODEL, "gmg_mg_score_reads: Score_All_Frames needs models of periodicity 3");
    if (reads->n_reads >= 0x7fffffffull) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: batch too large");
    if (!find_only && prm->nulls) {                     // classification mode: one null model per read
        if (!prm->read_null && reads->n_reads) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: nulls without read_null");
        for (uint64_t r = 0; r < reads->n_reads; r++)
            if (prm->read_null[r] >= (uint32_t)prm->nulls->n)
                return gmg_set_error(GMG_ERANGE, "gmg_mg_score_reads: read %llu names null model %u of %d", (unsigned long long)r,
                                     prm->read_null[r], prm->nulls->n);
    } else if (!find_only && (prm->read_null || prm->read_ignore_score_len))
        return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: read_null / read_ignore_score_len need a null set (gmg_mg_params.nulls)");
    const int err_mode = mg_err_mode(prm);
    if ((prm->flags & GMG_MG_ALLOW_INDELS) && (prm->flags & GMG_MG_ALLOW_SUBS))     // glimmer-mg.cc:952-955
        return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: cannot use indels and substitutions simultaneously");
    if (err_mode && (prm->indel_max < 0 || prm->indel_max > 2 || prm->indel_quality_threshold < 0 || prm->indel_quality_threshold > 254))
        return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: need indel_max in 0..2 and indel_quality_threshold in 0..254");
    const bool general = mg_general(prm);
    if (general && !find_only)
        return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: circular sequences / ignore regions are taken by gmg_find_orfs only");
    if (prm->n_ignore_regions < 0 || (prm->n_ignore_regions > 0 && (!prm->ignore_lo || !prm->ignore_hi)))
        return gmg_set_error(GMG_EINVAL, "gmg_find_orfs: n_ignore_regions without ignore_lo / ignore_hi");
    for (int k = 0; k < prm->n_ignore_regions; k++)     // as Get_Ignore_Regions leaves them: lo < hi, sorted, disjoint
        if (prm->ignore_lo[k] < 0 || prm->ignore_lo[k] >= prm->ignore_hi[k] || (k > 0 && prm->ignore_lo[k] < prm->ignore_hi[k - 1]))
            return gmg_set_error(GMG_EINVAL, "gmg_find_orfs: ignore region %d is not sorted / disjoint / lo < hi", k);
    return GMG_OK;
}

// the kernels' arguments as far as the host alone knows them: the batch, the thresholds, the codon sets, the error branch's penalties
static void mg_fill_args(MgArgs &a, double *pen_host, const gmg_reads *reads, const gmg_mg_params *prm, const int err_mode)
{
    memset(&a, 0, sizeof a);
    a.packed = reads->d_packed;
    a.read_off = reads->d_off;
    a.tile_read = reads->d_tile_read;
    a.n_reads = reads->n_reads;
    a.total = reads->total_bases;
    a.min_gene_len = prm->min_gene_len;
    a.allow_truncated = prm->allow_truncated;
    a.ignore_score_len = prm->ignore_score_len;
    a.start_threshold = prm->start_threshold;
    a.err_mode = err_mode;
    if (err_mode) {
        a.min_indel_orf_len = prm->min_indel_orf_len;
        a.indel_q_thr = prm->indel_quality_threshold;
        a.indel_max = prm->indel_max;
        a.indel_suffix_thr = prm->indel_suffix_score_threshold;
        for (int q = 0; q < 256; q++) {                 // Score_Indels (glimmer-mg.cc:1522-1523), the host's libm like the reference
            const double prob_err = pow(10.0, -(double)q / 10.0);
            pen_host[q] = log(prob_err / 2.0) - log(1.0 - prob_err);
        }
        for (int k = 0; k < 4; k++) {                   // Pass_Stop_Penalty (glimmer-mg.cc:961-995) without quality values
            const double default_p = 0.999;
            double p_stop = default_p;
            if (k & 2) p_stop *= 2.0 / 3.0 * default_p + 1.0 / 3.0; else p_stop *= default_p;
            if (k & 1) p_stop *= 2.0 / 3.0 * default_p + 1.0 / 3.0; else p_stop *= default_p;
            a.pass_stop[k] = log(1.0 - p_stop) - log(p_stop);
        }
    }
    {   // Set_Start_And_Stop_Codons (glimmer_base.cc:2683-2704) -> one bit / one byte per definite codon
        unsigned f_start[8], r_start[8], f_stop[8], r_stop[8];
        for (int p = 0; p < prm->n_start_codons; p++) { f_start[p] = mg_codon_from(prm->start_codon[p]); r_start[p] = mg_codon_revcomp(f_start[p]); }
        for (int p = 0; p < prm->n_stop_codons; p++) { f_stop[p] = mg_codon_from(prm->stop_codon[p]); r_stop[p] = mg_codon_revcomp(f_stop[p]); }
        for (unsigned idx = 0; idx < 64; idx++) {
            const unsigned data = (1u << ((idx >> 4) & 3)) << 8 | (1u << ((idx >> 2) & 3)) << 4 | (1u << (idx & 3));
            auto can_be = [&](const unsigned *pat, int np) {       // Codon_t::Can_Be (gene.cc:39-66)
                for (int p = 0; p < np; p++) { const unsigned x = data & pat[p]; if ((x & 0xf00) && (x & 0xf0) && (x & 0xf)) return p; }
                return -1;
            };
            auto must_be = [&](const unsigned *pat, int np) {      // Codon_t::Must_Be (gene.cc:70-92)
                for (int p = 0; p < np; p++) if ((data & pat[p]) == data) return true;
                return false;
            };
            a.which[idx] = (int8_t)can_be(f_start, prm->n_start_codons);
            if (a.which[idx] >= 0) a.fwd_start |= 1ull << idx;
            if (can_be(r_start, prm->n_start_codons) >= 0) a.rev_start |= 1ull << idx;
            if (must_be(f_stop, prm->n_stop_codons)) a.fwd_stop |= 1ull << idx;
            if (must_be(r_stop, prm->n_stop_codons)) a.rev_stop |= 1ull << idx;
        }
        for (unsigned v = 0; v < 64; v++) {
            const unsigned idx = (v & 3u) << 4 | (v & 12u) | v >> 4;
            if ((a.fwd_stop >> idx) & 1ull) a.fwd_stop_nat |= 1ull << v;
            if ((a.rev_stop >> idx) & 1ull) a.rev_stop_nat |= 1ull << v;
        }
    }
}

namespace {                     // (this translation unit's own: nothing of the driver is exported)

// Every decision about which kernels a call runs, made once from what the host knows before anything is queued: the models'
// exponents, the batch's statistics, the parameters and the options.  No HIP call, no allocation.
struct MgPlan {
    bool find_only = false, general = false, timing = false;
    int err_mode = 0, err_acc_only = 0;
    bool multi_stream = false;                          // Find_Orfs and the error branch's tables on side streams beside the main pass
    bool nul_dense3 = false;
    // Find_Orfs on bit masks (k_mg_find_orfs_bits) and its windows
    bool orf_bits = false;
    uint32_t ob_win_bases = 0, ob_rpw = 0, ob_grid = 1;
    uint64_t ob_windows = 0;
    // the table: GENE32 rows (g32) or the fp64 table of gmg_frame_score6
    bool g32 = false, err_g32 = false;
    // default mode, the running sums: tiles of cap bases (tiled), the reads no tile takes on the per-lane kernel (rest)
    int fused_nw = 0, fused_el = 9;                     // waves per tile of k_mg_tile_starts (0: the sequential kernels), elements per lane
    bool fused_nc2 = false;
    bool sums = false, small = false, tiled = false, rest = false;
    uint32_t cap = 0;
    int tile_reads_max = 0, reads_per_tile = 0;
    uint64_t tile_window = 0, n_windows = 0;
    // the error branch
    bool err_exact = false;                             // the batch's sums are exact in any order: the error branch may take differences of running sums
    bool err_tile = false;                              // ... and runs tile by tile with the sums in LDS (k_mg_err_tile)
    bool err_wave = false;                              // ... or with one wave per (read, strand), everything in the wave's LDS (k_mg_err_wave)
    uint32_t ew_cap = 0;
    // error branch, level by level: 0 (k_mg_err_level; the default), 1 = one lane per ORF with an explicit stack
    // (k_mg_err_flat: exact slots; the fallback of 0, and on its own with GMG_MG_ERR_FLAT=1 for A/B runs and cross-checks)
    int err_path = 0;
    int pfx = 0, qonly = 0, q454 = 0;                   // what MgArgs.pfx / .qonly / .q454 become where the level / wave kernels run
    uint32_t et_qcap = 0, et_ecap = 0, ew_qcap = 0;

    // reads shorter than this are walked by the wave / tile / level kernels, the others by k_mg_err_flat
    uint64_t err_fit_len() const { return err_wave ? (uint64_t)ew_cap + 1 : err_tile ? MG_ET_CAP + 1 : 2040; }

    // The fall-backs of the start lists' retry loop, in the order a batch can meet them:
    // a work-group's call slab / a wave's call stack was full: the batch repeats on the level kernels (they make the qualities themselves)
    void to_level_kernels() { err_tile = err_wave = false; q454 = 0; }
    // the level kernels' call arrays were too small and cannot grow: everything on the per-ORF kernel
    void to_per_orf_kernel() { err_path = 1; }
    // ... which walks the table itself: the GENE32 rows become the fp64 table (k_mg_apply_nulls)
    void to_fp64_table() { g32 = false; }
};

static MgPlan mg_plan(const gmg_model *gene, const gmg_model *nul, const MgGroups *groups, const gmg_reads *reads,
                      const gmg_mg_params *prm, const bool find_only, const bool own_table, const int no_wave)
{
    MgPlan p;
    const uint64_t n_reads = reads->n_reads, total = reads->total_bases;
    const int err_mode = mg_err_mode(prm);
    p.find_only = find_only;
    p.general = mg_general(prm);
    p.timing = gmg_opt(GMG_OPT_MG_TIMING) != 0;
    p.err_mode = err_mode;
    p.err_acc_only = (prm->flags & GMG_MG_ACCEPTED_ONLY) ? 1 : 0;
    p.multi_stream = !find_only && !p.timing && !gmg_opt(GMG_OPT_MG_ONE_STREAM);
    p.err_path = gmg_opt(GMG_OPT_MG_ERR_FLAT) ? 1 : 0;
    p.et_qcap = gmg_opt(GMG_OPT_MG_ERR_TILE_Q) > 0 ? (uint32_t)gmg_opt(GMG_OPT_MG_ERR_TILE_Q) : (uint32_t)ET_QCAP;
    p.et_ecap = gmg_opt(GMG_OPT_MG_ERR_TILE_Q) > 0 ? (uint32_t)(4 * gmg_opt(GMG_OPT_MG_ERR_TILE_Q)) : (uint32_t)ET_ECAP;
    p.ew_qcap = gmg_opt(GMG_OPT_MG_ERR_WAVE_Q) > 0 ? (uint32_t)gmg_opt(GMG_OPT_MG_ERR_WAVE_Q) : (uint32_t)EW_QCAP;
    // Find_Orfs on bit masks (k_mg_find_orfs_bits): a wave per window of whole reads under its OB_WORDS x 32 bases, ten reads at a time.
    // Uniform batches: up to ten reads per window; ragged ones: the reads that begin in a stretch of about ten mean read lengths (and
    // no more than the window holds with the longest read at its end).  Not with reads beyond OB_MAX_LEN.
    p.orf_bits = !p.general && n_reads && total && gmg_opt(GMG_OPT_MG_ORFS_BITS) && reads->max_len <= OB_MAX_LEN && reads->max_len > 0;
    if (p.orf_bits) {
        if (reads->uniform_len > 0) {
            p.ob_rpw = (uint32_t)((OB_SPAN - 31) / reads->uniform_len);
            if (p.ob_rpw > OB_GROUP) p.ob_rpw = OB_GROUP;
            p.ob_windows = (n_reads + p.ob_rpw - 1) / p.ob_rpw;
        } else {
            const uint64_t room = OB_SPAN - 31 - reads->max_len, want = (total * 19 / 2) / n_reads;      // 9.5 mean lengths
            p.ob_win_bases = (uint32_t)(want < room ? (want > 0 ? want : 1) : room);
            p.ob_windows = (total + p.ob_win_bases - 1) / p.ob_win_bases;
        }
        const uint64_t blocks = (p.ob_windows + OB_WAVES - 1) / OB_WAVES;
        p.ob_grid = (uint32_t)(blocks < 256 * 32 ? blocks : 256 * 32);
    }
    if (find_only) return p;

    const long long forced_tile = gmg_opt(GMG_OPT_MG_TILE);
    // The call's own table in the default mode is the GENE32 form: the gene model's fp32 rows (half the bytes to write, half to
    // read back), the null model applied where the running sums are built.  A caller's table, the error branch (its walks read
    // the table in place) and model shapes without the fast path keep the fp64 table of gmg_frame_score6.
    p.nul_dense3 = nul->dev.has_dense && nul->dev.W == 3 && nul->dev.P == 3 && nul->dev.dense_part == nul->dev.dense + 192;
    // Measured (1M x 500 bp, profiles/r02_mg_*): with ONE null model the fp64 table wins (running sums 7.2 ms against 9.1 ms: the
    // conversion costs more vector work than the halved read saves); with per-read null models GENE32 saves the extra pass over
    // the table (13.3 ms against 16.6 ms for the table + sums).  Option mg_gene32: 0 never, 1 with per-read nulls and with tiles of two waves or more (default), 2 always.
    // The fused kernel (k_mg_tile_starts: sums as a parallel scan + start lists) when every sum of the batch is exact in any
    // order -- see there; R = the longest read + 2 terms.
    {
        const int n_min = prm->nulls ? prm->nulls->min_exp : nul->min_exp, n_max = prm->nulls ? prm->nulls->max_exp : nul->max_exp;
        const int n_odd = prm->nulls ? prm->nulls->odd_values : nul->odd_values;
        int g_min = gene->min_exp, g_max = gene->max_exp, g_odd = gene->odd_values;
        for (int k = 0; groups && k < groups->n; k++) {   // every group's model
            const gmg_model *m = groups->models[k];
            if (m->min_exp < g_min) g_min = m->min_exp;
            if (m->max_exp > g_max) g_max = m->max_exp;
            g_odd |= m->odd_values;
        }
        const int mn = g_min < n_min ? g_min : n_min, mx = g_max > n_max ? g_max : n_max;
        int clog = 0;
        const uint64_t longest_read = reads->max_len ? reads->max_len : reads->total_bases;   // (no lengths on the host: the batch's size is a bound)
        while ((1ull << clog) < longest_read + 2) clog++;
        const bool exact = !g_odd && !n_odd && (mx < mn || clog + mx - mn <= 28);
        p.err_exact = exact;
        if (!err_mode && exact && gmg_opt(GMG_OPT_MG_FUSED) && n_reads && total) {
            if (forced_tile == 1 || forced_tile == 2 || forced_tile == 4) p.fused_nw = (int)forced_tile;
            else if (reads->uniform_len > 0) p.fused_nw = reads->uniform_len <= MT_W ? 1 : reads->uniform_len <= 2 * MT_W ? 2 : reads->uniform_len <= 4 * MT_W ? 4 : 0;
            else p.fused_nw = (reads->max_len <= MT_W || reads->n_over_512 * 10 <= reads->n_reads) ? 1 : reads->max_len <= 2 * MT_W ? 2 : 4;
            if (reads->uniform_len > (int)(MT_W * p.fused_nw)) p.fused_nw = 0;
            // Measured (1M reads, tests/bench/bench_mg.py with GMG_MG_TILE; profiles/r02_mg_tile_width.txt): ragged reads fill four-wave tiles
            // better than one-wave ones (~400 bp: 70 % of 567 bases, 88 % of 2,268) -- 12.5 -> 11.7 ms with one null model, 13.7 -> 10.95 ms with
            // a null model per read (one LDS table per read and tile: fewer, fuller tiles); two-wave tiles for uniform batches (two 500-bp reads
            // per tile): 12.3 -> 11.1 ms with a null model per read, 11.1 -> 10.9 ms with one (fp64 table), 11.5 -> 10.2 ms with the GENE32
            // table, which is why the call's own table takes that form whenever the tiles have two waves or more.
            // (A tile takes whole reads, at most tile_reads_max of them.)
            if (!(forced_tile == 1 || forced_tile == 2 || forced_tile == 4) && p.fused_nw) {
                const uint64_t mean = total / n_reads, per_tile = prm->nulls ? MT_NC : MG_TILE_READS;
                if (reads->uniform_len == 0 && mean * per_tile * 5 >= (uint64_t)4 * MT_W * 4) p.fused_nw = 4;
                else if (reads->uniform_len > 0 && p.fused_nw == 1 && (uint64_t)reads->uniform_len * per_tile >= (uint64_t)2 * MT_W) p.fused_nw = 2;
            }
            // eight elements per lane (504 bases per wave) when the reads of a uniform batch fill such tiles as well as the larger ones
            if (p.fused_nw && reads->uniform_len > 0) {
                const int l = reads->uniform_len, c8 = 504 * p.fused_nw, c9 = (int)MT_W * p.fused_nw;
                if (l <= c8 && (c8 / l) * 9 >= (c9 / l) * 8) p.fused_el = 8;
            }
            // ragged batches too when no read needs the wider tile: the eight-element form runs four waves per SIMD (9.76 -> 9.54 ms per 1 M x ~400 bp)
            else if (p.fused_nw && reads->max_len && reads->max_len <= (uint64_t)504 * p.fused_nw) p.fused_el = 8;
        }
    }
    // (the fused kernel reads whichever table there is.  Measured, 1M x 500 bp, one null model: the fp64 table 4.9 + 6.2 ms, the
    // GENE32 form 3.9 + 7.5 ms -- the kernel is bound by its vector instructions, not by the table's bytes, and the null-model
    // lookups add a quarter to them; profiles/r02_mg_pmc_*.txt)
    const long long g32_opt = gmg_opt(GMG_OPT_MG_GENE32);
    // (with tiles of two waves or more the GENE32 form wins with one null model as well: ragged 10.6 -> 10.0 ms per 1M x ~400 bp,
    // 500-bp reads 10.9 -> 10.2 ms)
    bool all_fast = gmg_f6_shape(gene->dev);
    for (int k = 0; groups && k < groups->n; k++) {
        const GmgDevModel &m = groups->models[k]->dev;
        all_fast = all_fast && gmg_f6_shape(m) && m.W == gene->dev.W;
    }
    // (groups of any-shape models: their gene rows come from the exact kernel, group by group -- still the GENE32 form)
    // the error branch on running sums (mg_err_skip) never reads the table itself, only the walk-order sums made from it: the
    // gene rows as fp32 (GENE32) then save the 48 B/base table's write and half of what the sums' kernel reads.  Not with reads the
    // level kernels cannot take (>= 2040 bases: k_mg_err_flat walks the table) or a forced per-ORF path; a call-array overflow
    // builds the table then (k_mg_apply_nulls) before it falls back.
    // the error branch tile by tile (k_mg_err_tile: the running sums in LDS) wants what the running-sum form wants; reads longer than
    // a tile go to k_mg_err_flat, which walks the fp64 table
    // Which of the two: measured on ragged ~400-bp reads (profiles/r04_errtile_crossover.txt), the tile kernel -- ONE launch, no table in
    // HBM -- wins on batches up to ~200,000 reads (-i: 1.1 vs 2.4 ms at 5,000 reads, 3.4 vs 4.7 at 50,000, 11.3 vs 11.6 at 200,000), the
    // level kernels from there on (22.1 vs 21.2 ms at 400,000, 54.3 vs 48.6 at 1M).  mg_err_tile: -1 (default) by the batch's size,
    // 1 always, 0 never.
    const long long tile_opt = gmg_opt(GMG_OPT_MG_ERR_TILE);
    const bool tile_wanted = tile_opt > 0 || (tile_opt < 0 && total <= (err_mode == 1 ? (uint64_t)MG_ET_AUTO_BASES_INDEL : (uint64_t)MG_ET_AUTO_BASES_SUB));
    p.err_tile = err_mode && p.err_exact && gmg_opt(GMG_OPT_MG_ERR_SKIP) && tile_wanted && !gmg_opt(GMG_OPT_MG_ERR_FLAT);
    // one wave per (read, strand) (k_mg_err_wave; the default whenever the sums are exact, unless the tile kernel is forced):
    // its LDS share is sized by the batch's longest read, reads beyond EW_MAX_CAP go to k_mg_err_flat
    // mg_err_wave: 1 (default), 2 = with the stack walker as the count pass too (cross-check), 0 = the tile / level kernels
    p.err_wave = err_mode && p.err_exact && gmg_opt(GMG_OPT_MG_ERR_SKIP) && !gmg_opt(GMG_OPT_MG_ERR_FLAT) && gmg_opt(GMG_OPT_MG_ERR_WAVE) > 0 &&
               !no_wave && tile_opt <= 0 && reads->max_len > 0 && total;
    if (p.err_wave) {
        p.err_tile = false;
        const uint64_t longest = reads->max_len < EW_MAX_CAP ? reads->max_len : EW_MAX_CAP;
        p.ew_cap = (uint32_t)((longest + 63) & ~63ull);
    }
    p.err_g32 = err_mode && own_table && total && g32_opt != 0 && p.nul_dense3 && all_fast && p.err_exact &&
                         gmg_opt(GMG_OPT_MG_ERR_SKIP) && !gmg_opt(GMG_OPT_MG_ERR_FLAT) && reads->max_len && reads->max_len < p.err_fit_len();
    p.g32 = p.err_g32 || (own_table && !err_mode && total &&
                     (g32_opt == 2 || (g32_opt == 1 && (prm->nulls || p.fused_nw >= 2))) && p.nul_dense3 &&
                     (all_fast || (groups && groups->n > 0)));
    // the error branch's own choices where the level / wave kernels run
    p.pfx = p.err_exact && gmg_opt(GMG_OPT_MG_ERR_SKIP) ? 1 : 0;
    // -s on running sums: one value per base and strand is all its walks read (16 B/base instead of 48: a third of the table to
    // write, a third to keep in the caches)
    p.qonly = err_mode == 2 && gmg_opt(GMG_OPT_MG_ERR_QONLY) ? 1 : 0;
    // The wave kernels compute Set_Quality_454 themselves from the bases they hold (no quality file, every read short enough for them):
    // no quality kernel, no 2 B/base of quality arrays written and read back; a fall-back to the level kernels makes them then
    p.q454 = err_mode == 1 && p.err_wave && !prm->quality && reads->max_len <= (uint64_t)p.ew_cap && gmg_opt(GMG_OPT_MG_ERR_WAVE) != 0 ? 1 : 0;

    p.sums = !err_mode && n_reads && total;
    if (p.sums) {
        // tile shape of the sequential kernel: two waves and <= 512 bases (12 KB of LDS, many blocks per CU in different phases)
        // when the reads allow it, else eight waves and 1504 bases (39.8 KB, four blocks per CU); the fused kernel: 567 bases per wave
        // (ragged batches: the few reads beyond 512 bases go to the per-lane kernel; measured 9.6 vs 10.6 ms on 1M x ~400 bp)
        p.small = forced_tile ? forced_tile == 512 : (reads->max_len <= 512 || (reads->uniform_len == 0 && reads->n_over_512 * 10 <= reads->n_reads));
        p.cap = p.fused_nw ? (uint32_t)(3 * MT_CL * p.fused_el * p.fused_nw) : p.small ? 512 : 1504;
        p.tile_reads_max = p.fused_nw && p.g32 && prm->nulls ? MT_NC : MG_TILE_READS;
        // (two-wave tiles of eight elements over uniform reads of which two at most fit: the kernel form with two null tables)
        p.fused_nc2 = p.fused_nw == 2 && p.fused_el == 8 && p.g32 && prm->nulls && reads->uniform_len > 0 && p.cap / (uint32_t)reads->uniform_len <= 2;
        if (p.fused_nc2) p.tile_reads_max = 2;
        p.rest = true;
        if (reads->uniform_len > 0) {                  // every tile takes cap / L whole reads
            if ((uint32_t)reads->uniform_len <= p.cap) {
                p.reads_per_tile = (int)(p.cap / reads->uniform_len) < p.tile_reads_max ? p.cap / reads->uniform_len : p.tile_reads_max;
                p.tiled = true; p.rest = false;
            }
        } else {                                        // the reads that start inside a window of tile_window bases
            const uint64_t longest = reads->max_len < p.cap / 2 ? reads->max_len : p.cap / 2;
            p.tile_window = p.cap - longest;
            p.n_windows = total / p.tile_window + 1;
            p.tiled = true;
            p.rest = reads->max_len > longest || reads->min_len * (uint64_t)p.tile_reads_max < p.tile_window;
        }
        if (p.fused_nw && !p.tiled) p.fused_nw = 0;
    }
    return p;
}

// The side streams of one (host thread, device), made when a call first needs them and kept: a set counts as made only when all
// of it exists.  The set is the thread's (thread_local, below): when the thread ends its destructor gives streams and events back,
// as Thread_Staging_t (host/icm.cc) does with the thread's staging.  No call of the thread is running then, and every call has
// joined the side streams into the caller's stream and waited for that one (MgRun::finish), so nothing is queued on them.
template <int NS, int NE>
struct MgStreamSet {
    hipStream_t st[NS] = {};
    hipEvent_t ev[NE] = {};
    bool made = false;
    MgStreamSet() {}
    MgStreamSet(const MgStreamSet &) = delete;
    MgStreamSet &operator=(const MgStreamSet &) = delete;
    ~MgStreamSet()
    {
        if (!made) return;
        drop();                                         // (the main thread's set goes at process exit: whatever HIP answers then is ignored)
        g_gmg_thread_streams -= NS + NE;
    }
    hipError_t need(const bool low_priority, const int prio)
    {
        if (made) return hipSuccess;
        hipError_t e = hipSuccess;
        for (int k = 0; k < NS && e == hipSuccess; k++)
            e = low_priority ? hipStreamCreateWithPriority(&st[k], hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking);
        for (int k = 0; k < NE && e == hipSuccess; k++) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
        made = e == hipSuccess;
        if (made) g_gmg_thread_streams += NS + NE;
        else drop();
        return e;
    }
private:
    void drop()
    {
        for (int k = 0; k < NS; k++) { if (st[k]) (void)hipStreamDestroy(st[k]); st[k] = nullptr; }
        for (int k = 0; k < NE; k++) { if (ev[k]) (void)hipEventDestroy(ev[k]); ev[k] = nullptr; }
        made = false;
    }
};
struct MgStreams {
    MgStreamSet<1, 2> side;      // Find_Orfs beside the main pass; ev: its work is done, the caller's running sums are done
    MgStreamSet<1, 1> side2;     // error branch: the qualities and the run lengths beside the ORF scan and the six-frame table
    MgStreamSet<4, 5> cls;       // the wave kernels' length classes: ev[k]: class k + 1 is done, ev[4]: the fork
};
static thread_local MgStreams tl_mg_streams[16];        // one per device this host thread has used

#define MG_TRY(call)                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess)                                                                                   \
            return gmg_set_error(e_ == hipErrorOutOfMemory ? GMG_ENOMEM : GMG_EHIP, "gmg_mg_score_reads: %s: %s", \
                                 #call, hipGetErrorString(e_));                                                 \
    } while (0)
#define MG_STAGE(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// One call.  Whichever way run() returns, ~GmgScratch gives back every block the result has not taken -- after a wait for the
// whole device unless the call succeeded (the side streams and the class streams may still be running; on success the wait for
// the caller's stream in finish() is the point behind which nothing uses them).
struct MgRun {
    const gmg_model *gene, *nul;
    const gmg_reads *reads;
    const gmg_mg_params *prm;
    const MgGroups *groups;
    double *d_frame_scores;                             // the table: the caller's, or the call's own
    hipStream_t s, s2, s3;                              // the caller's stream; the side streams (= s without them)
    MgStreams *streams = nullptr;
    int dev_id = 0;
    MgArgs a;
    MgPlan p;
    GmgScratch sc;
    MgTimer &tm;
    gmg_mg_result *res = nullptr;
    double pen_host[256];
    uint64_t nr = 0, no = 0;
    const float *d_null_tab = nullptr;
    double *d_fs_own = nullptr, *d_cum = nullptr, *d_pen = nullptr, *d_walk = nullptr;
    float *d_gene32 = nullptr;
    uint32_t *d_read_null = nullptr, *d_read_cnt = nullptr, *d_orf_cnt = nullptr, *d_unfit = nullptr;
    int32_t *d_read_isl = nullptr;
    uint64_t *d_start_off = nullptr, *d_keys = nullptr;
    uint8_t *d_qual = nullptr, *d_user_q = nullptr, *d_read_fit = nullptr, *d_walk_q = nullptr, *d_run = nullptr, *d_item_flag = nullptr;
    uint32_t *d_err_flag = nullptr, *d_fill = nullptr, *d_acc_bits = nullptr;
    MgCall *d_calls[2] = {nullptr, nullptr};
    MgOrfAgg *d_agg = nullptr;
    // k_mg_err_tile: work-groups (ET_WG_PER_CU per CU: sizeof (EtLds<MG_ET_CAP>) of LDS each), their slabs (calls per level, starts per batch of ORFs), the tile
    // list, the staging arrays (the kept ORFs' slices in the order the tiles finish)
    MgTile *d_et_tiles = nullptr;
    MgCall *d_et_slabs = nullptr;
    EtEm *d_et_em = nullptr;
    gmg_start *d_st_s = nullptr;
    gmg_start_errors *d_st_e = nullptr;
    uint64_t *d_st_k = nullptr;
    unsigned et_grid = 0;
    uint64_t et_stage_cap = 0;
    uint32_t *d_et_ntiles = nullptr;
    unsigned long long *d_et_items = nullptr, *d_et_stage_ctr = nullptr;
    bool wave_reset_done = false;

    MgRun(const gmg_model *gene_, const gmg_model *nul_, const gmg_reads *reads_, const gmg_mg_params *prm_, double *d_frame_scores_,
          hipStream_t s_, const bool find_only, const MgGroups *groups_, MgTimer &tm_)
        : gene(gene_), nul(nul_), reads(reads_), prm(prm_), groups(groups_), d_frame_scores(d_frame_scores_), s(s_), s2(s_), s3(s_), tm(tm_)
    {
        p = mg_plan(gene, nul, groups, reads, prm, find_only, !d_frame_scores, tl_mg_no_wave);
        mg_fill_args(a, pen_host, reads, prm, p.err_mode);
        nr = a.n_reads;
        sc.wait = GmgScratch::DEVICE;
    }
    ~MgRun() { delete res; }                            // (its arrays are the scratch's until run() hands them over)

    int run(gmg_mg_result **out)
    {
        res = new (std::nothrow) gmg_mg_result();
        if (!res) { sc.wait = GmgScratch::NONE; return gmg_set_error(GMG_ENOMEM, "gmg_mg_score_reads: out of host memory"); }
        res->n_reads = reads->n_reads;
        res->s = s;
        if (!p.find_only) {                                 // 1. Frame_Scores
            if (prm->nulls && !p.nul_dense3) return gmg_set_error(GMG_EBADMODEL, "gmg_mg_score_reads: per-read null models are (3,2,3) models");
            MG_STAGE(upload_tables());
            MG_STAGE(frame_scores());
            MG_STAGE(running_sums());
        }
        MG_STAGE(side_streams());                           // 2. ORFs of every read
        MG_STAGE(find_orfs());
        if (!p.find_only) {
            MG_STAGE(err_tables());
            MG_STAGE(start_lists());                        // 3. start lists
            if (p.err_acc_only) MG_STAGE(pack_accepted());  // 4.
        }
        MG_STAGE(push_order());                             // 5.
        MG_STAGE(finish());
        res->own.take(sc, res->d_orfs); res->own.take(sc, res->d_starts); res->own.take(sc, res->d_read_orf_off); res->own.take(sc, res->d_errs);
        sc.wait = GmgScratch::NONE;
        *out = res;
        res = nullptr;
        return GMG_OK;
    }

    // the per-call host tables: penalties, the reads' null models and Ignore_Score_Len values
    int upload_tables()
    {
        if (p.err_mode) {
            // the penalties go up FIRST: behind the six-frame kernels this 2 KB copy waited a millisecond for a free slot beside the
            // side streams' kernels, and the running sums behind it (profiles/r03_mgerr_timeline_indel.txt of the build before)
            MG_TRY(sc.alloc(&d_pen, sizeof pen_host));
            MG_TRY(hipMemcpyAsync(d_pen, pen_host, sizeof pen_host, hipMemcpyHostToDevice, s));    // (pen_host lives as long as the run)
            a.pen = d_pen;
        }
        // classification mode: the per-read tables go to the device once per call (4 + 4 bytes per read)
        // (a (3,2,3) model's partial-window table follows its full-window table in the model blob: gmg_model_upload)
        d_null_tab = nul->dev.dense;
        if (prm->nulls) {
            d_null_tab = prm->nulls->d_tab;
            if (a.n_reads) {
                MG_TRY(sc.alloc(&d_read_null, a.n_reads * 4));
                MG_TRY(hipMemcpyAsync(d_read_null, prm->read_null, a.n_reads * 4, hipMemcpyHostToDevice, s));
                if (prm->read_ignore_score_len) {
                    MG_TRY(sc.alloc(&d_read_isl, a.n_reads * 4));
                    MG_TRY(hipMemcpyAsync(d_read_isl, prm->read_ignore_score_len, a.n_reads * 4, hipMemcpyHostToDevice, s));
                }
            }
            a.read_null = d_read_null;
            a.read_isl = d_read_isl;
        }
        a.null_tab = d_null_tab;
        return GMG_OK;
    }

    // the table: GENE32 rows, or the fp64 table (the call's own, or the caller's)
    int frame_scores()
    {
        a.fs_stride = a.total;
        if (p.g32) {
            a.fs_stride = (a.total + 31) & ~31ull;          // every fp32 row on a 128-byte line
            // (64 spare floats on both sides: the wave kernels of the error branch load their lanes' steps without predicates)
            MG_TRY(sc.alloc(&d_gene32, ((size_t)6 * a.fs_stride + 128) * sizeof(float)));
            MG_STAGE(mg_gene6_full(gene, groups, reads, d_gene32 + 64, a.fs_stride, s));
            a.gene32 = d_gene32 + 64;
            a.ew_slack = 1;
        } else {
            if (!d_frame_scores && a.total) {
                a.fs_stride = (a.total + 15) & ~15ull;      // our own table: every row on a 128-byte line
                MG_TRY(sc.alloc(&d_fs_own, (size_t)6 * a.fs_stride * sizeof(double)));
                d_frame_scores = d_fs_own;
            }
            if (a.total) {
                if (prm->nulls) MG_STAGE(mg_frame6_nulls(gene, d_null_tab, d_read_null, reads, d_frame_scores, a.fs_stride, s, groups));
                else MG_STAGE(gmg_launch_frame6_strided(gene, nul, reads, d_frame_scores, a.fs_stride, s));
            }
            a.fs = d_frame_scores;
        }
        tm.lap("frame scores");
        if (p.err_mode == 1 && a.total) {                   // the error branch sums per call; it needs the penalties and the qualities
            MG_TRY(sc.alloc(&d_qual, a.total + 8 + 128));   // (+8: the level kernels read four values at a time; 64 spare bytes on both sides)
            if (prm->quality) MG_TRY(sc.alloc(&d_user_q, a.total));
            a.qual = d_qual + 64;                           // filled in find_orfs(), beside Find_Orfs on the second stream
        }
        return GMG_OK;
    }

    // ragged batches: the tile of every window of tile_window bases, and the non-empty ones as a list
    int tile_table()
    {
        const uint64_t n_windows = p.n_windows;
        if (n_windows >= 0x7fffffffull) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_reads: batch too large");
        MgTile *d_tiles = nullptr, *d_all = nullptr;
        uint32_t *d_n = nullptr, *d_flag = nullptr;         // d_flag: [n_windows + 1] flags, then [n_windows + 1] their exclusive sums
        MG_TRY(sc.alloc(&d_all, n_windows * sizeof(MgTile)));
        MG_TRY(sc.alloc(&d_tiles, n_windows * sizeof(MgTile)));
        MG_TRY(sc.alloc(&d_n, 4));
        MG_TRY(sc.alloc(&d_flag, (2 * (n_windows + 4)) * 4));
        uint32_t *d_pos = d_flag + ((n_windows + 4) & ~3ull);
        hipLaunchKernelGGL(k_mg_tile_table, dim3(grid_for(n_windows)), dim3(256), 0, s, a, n_windows, p.cap, d_all);
        hipLaunchKernelGGL(k_mg_tile_flags, dim3(grid_for(n_windows + 1)), dim3(256), 0, s, d_all, n_windows, d_flag);
        MG_TRY((gmg_scan_excl<uint32_t, uint32_t>(d_flag, d_pos, n_windows + 1, s)));
        hipLaunchKernelGGL(k_mg_tile_compact, dim3(grid_for(n_windows)), dim3(256), 0, s, d_all, n_windows, d_pos, d_tiles, d_n);
        MG_TRY(hipGetLastError());
        a.tiles = d_tiles;
        a.windows = d_all;
        a.n_tiles_dev = d_n;
        a.n_tiles = n_windows;                              // upper bound, for the grid
        return GMG_OK;
    }

    // the reads no tile takes, as a list for the per-lane kernels
    int list_unfit()
    {
        a.lanes_only_unfit = 1;
        MG_TRY(sc.alloc(&d_unfit, (a.n_reads + 1) * 4));
        a.unfit = d_unfit + 1;
        a.unfit_n = d_unfit;
        MG_TRY(hipMemsetAsync(d_unfit, 0, 4, s));
        hipLaunchKernelGGL(k_mg_unfit_list, dim3(grid_for(a.n_reads)), dim3(256), 0, s, a);
        MG_TRY(hipGetLastError());
        return GMG_OK;
    }

    void launch_cum()
    {
        if (p.g32) hipLaunchKernelGGL(k_mg_cum<true>, dim3(grid_for(2 * a.n_reads)), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_mg_cum<false>, dim3(grid_for(2 * a.n_reads)), dim3(256), 0, s, a);
    }

    // running sums of every reading-frame class (what Cumulative_Frame_Score would give any ORF)
    int running_sums()
    {
        if (p.sums) {
            const uint32_t cap = p.cap;
            a.tile_cap = (int)cap;
            a.tile_reads_max = p.tile_reads_max;
            if (reads->uniform_len > 0) {                   // every tile takes cap / L whole reads
                if (p.tiled) {
                    a.uniform_len = reads->uniform_len;
                    a.uniform_magic = (uint32_t)((0x100000000ull + (uint64_t)reads->uniform_len - 1) / (uint64_t)reads->uniform_len);
                    a.reads_per_tile = p.reads_per_tile;
                    a.n_tiles = (a.n_reads + a.reads_per_tile - 1) / a.reads_per_tile;
                }
            } else {                                        // the reads that start inside a window of tile_window bases
                a.tile_window = p.tile_window;
                MG_STAGE(tile_table());
            }
            if (!p.fused_nw || p.rest) {
                MG_TRY(sc.alloc(&d_cum, (size_t)2 * a.total * sizeof(double)));
                a.cum = d_cum;
            }
            if (p.fused_nw) {
                // the kernel itself goes behind the ORF scan and the count pass (it writes the start lists); the reads no tile takes are
                // listed now
                if (p.rest) {
                    MG_STAGE(list_unfit());
                    launch_cum();
                    MG_TRY(hipGetLastError());
                }
            } else {
                if (p.tiled && a.n_tiles) {
                    const size_t lds = (size_t)3 * (cap + 8) * sizeof(double);
                    const unsigned grid = (unsigned)(2 * a.n_tiles < 256 * 1024 ? 2 * a.n_tiles : 256 * 1024);
                    if (p.small) {                          // two waves per tile: 7.1 ms; one: 8.0; four: 9.0
                        if (p.g32) hipLaunchKernelGGL((k_mg_cum_tiled<512, 128, true>), dim3(grid), dim3(128), lds, s, a);
                        else hipLaunchKernelGGL((k_mg_cum_tiled<512, 128, false>), dim3(grid), dim3(128), lds, s, a);
                    } else {
                        // eight waves per tile: 8.8 ms per 400k x 1000 bp; four: 9.7; two: 11.1; twelve: 13.3
                        if (p.g32) {
                            MG_TRY(hipFuncSetAttribute((const void *)k_mg_cum_tiled<1504, 512, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                            hipLaunchKernelGGL((k_mg_cum_tiled<1504, 512, true>), dim3(grid), dim3(512), lds, s, a);
                        } else {
                            MG_TRY(hipFuncSetAttribute((const void *)k_mg_cum_tiled<1504, 512, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                            hipLaunchKernelGGL((k_mg_cum_tiled<1504, 512, false>), dim3(grid), dim3(512), lds, s, a);
                        }
                    }
                    MG_TRY(hipGetLastError());
                }
                if (p.rest) {
                    if (p.tiled && a.windows != nullptr) MG_STAGE(list_unfit());
                    launch_cum();
                    MG_TRY(hipGetLastError());
                }
            }
        }
        tm.lap("running sums");
        return GMG_OK;
    }

    // Find_Orfs and the count pass of the start scan need only the packed reads: they run on a second stream beside the six-frame
    // and running-sum kernels (light kernels without LDS, they fit next to the main pass's work-groups) and join the caller's
    // stream before the start lists are written.
    int side_streams()
    {
        MG_TRY(hipGetDevice(&dev_id));
        if (!p.multi_stream || dev_id < 0 || dev_id >= 16) return GMG_OK;
            // (the side streams get the lowest priority: their kernels fill the gaps of the caller's stream and must not keep its short
            // kernels waiting -- k_frame6p, 0.45 ms alone, took 5.9 ms beside the error branch's side kernels at equal priority)
        int prio_least = 0, prio_greatest = 0;
        MG_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        MgStreams &ts = tl_mg_streams[dev_id];
        MG_TRY(ts.side.need(true, prio_least));
        streams = &ts;
        s2 = s3 = ts.side.st[0];
        if (p.err_mode) {
            MG_TRY(ts.side2.need(true, prio_least));
            s3 = ts.side2.st[0];
        }
        return GMG_OK;
    }

    // Set_Quality_454 / Clean_Quality_454: needs the reads only
    int build_qualities(hipStream_t st)
    {
        if (prm->quality) MG_TRY(hipMemcpyAsync(d_user_q, prm->quality, a.total, hipMemcpyHostToDevice, st));
        if (!d_walk_q) MG_TRY(sc.alloc(&d_walk_q, a.total + 8));
        hipLaunchKernelGGL(k_mg_quality, dim3(grid_for(nr * 64)), dim3(256), 0, st, a, d_user_q, d_qual + 64, d_walk_q);
        a.walk_q = d_walk_q;
        MG_TRY(hipGetLastError());
        return GMG_OK;
    }

    // ORF discovery: count, scan, write (one lane per read / events / bit masks / the general form with ignore regions and circular sequences)
    int find_orfs()
    {
        // (in front of the ORF scan's count pass: behind it the launch waited for the host to come back from the scan's total -- it then
        // ran beside the ORF write pass, both at half speed, 1 ms on the error branch's critical path; here it runs in the six-frame
        // kernel's shadow: no LDS, few registers)
        a.q454 = p.q454;
        if (p.err_mode == 1 && a.total && !p.find_only && !a.q454) {
            MG_STAGE(build_qualities(s3));
            tm.lap("quality values");
        }
        MG_TRY(sc.alloc(&d_read_cnt, (nr + 1) * 4));
        MG_TRY(hipMemsetAsync(d_read_cnt, 0, (nr + 1) * 4, s2));
        MG_TRY(sc.alloc(&res->d_read_orf_off, (nr + 1) * 8));
        a.read_cnt = d_read_cnt;
        int32_t *d_ign = nullptr;                           // general form: the regions' lo values, then their hi values; [2 n]: the failure flag
        const int n_ign = p.general ? prm->n_ignore_regions : 0;
        if (p.general) {
            MG_TRY(sc.alloc(&d_ign, (size_t)(2 * n_ign + 1) * 4));
            if (n_ign) {
                MG_TRY(hipMemcpyAsync(d_ign, prm->ignore_lo, (size_t)n_ign * 4, hipMemcpyHostToDevice, s2));
                MG_TRY(hipMemcpyAsync(d_ign + n_ign, prm->ignore_hi, (size_t)n_ign * 4, hipMemcpyHostToDevice, s2));
            }
            MG_TRY(hipMemsetAsync(d_ign + 2 * n_ign, 0, 4, s2));
            if (nr) hipLaunchKernelGGL(k_find_orfs_general<false>, dim3(grid_for(nr)), dim3(64), 0, s2, a, prm->circular ? 1 : 0, n_ign, d_ign, d_ign + n_ign,
                                       (uint32_t *)(d_ign + 2 * n_ign));
        } else if (p.orf_bits) {
            hipLaunchKernelGGL(k_mg_find_orfs_bits<false>, dim3(p.ob_grid), dim3(64 * OB_WAVES), 0, s2, a, p.ob_windows, p.ob_win_bases, p.ob_rpw);
        } else if (nr) hipLaunchKernelGGL(k_mg_find_orfs<false>, dim3(grid_for(nr)), dim3(256), 0, s2, a);
        MG_TRY(hipGetLastError());
        MG_STAGE(mg_scan(d_read_cnt, res->d_read_orf_off, nr, &res->n_orfs, s2));
        if (res->n_orfs > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
            return gmg_set_error(GMG_ETOOBIG, "gmg_mg_score_reads: %llu ORFs in one batch, the result's 32-bit fields hold %lld: split the batch",
                                 (unsigned long long)res->n_orfs, gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
        no = res->n_orfs;
        MG_TRY(sc.alloc(&res->d_orfs, (no ? no : 1) * sizeof(gmg_mg_orf)));
        a.read_orf_off = res->d_read_orf_off;
        a.orfs = res->d_orfs;
        a.n_orfs = no;
        {   // default mode: the write pass of the ORF scan counts every ORF's starts as it goes (lowest j within the 64 codons its mask holds)
            const int j_lo = ((a.min_gene_len - 3 > 1 ? a.min_gene_len - 3 : 1) + 2) / 3 * 3;
            a.count_starts = !p.find_only && !p.err_mode && 1 + j_lo / 3 <= 64;
            if (!p.find_only) {
                MG_TRY(sc.alloc(&d_orf_cnt, (no + 1) * 4));
                // (the counting write pass stores every ORF's count itself: only the scan's extra element needs a zero -- the 30 MB
                // memset sat 0.26 ms on the critical path, in front of the write pass)
                if (!a.count_starts || nr == 0) MG_TRY(hipMemsetAsync(d_orf_cnt, 0, (no + 1) * 4, s2));   // (else the write pass zeroes the last element)
                a.orf_cnt = d_orf_cnt;
            }
        }
        if (p.general) {
            if (nr) hipLaunchKernelGGL(k_find_orfs_general<true>, dim3(grid_for(nr)), dim3(64), 0, s2, a, prm->circular ? 1 : 0, n_ign, d_ign, d_ign + n_ign,
                                       (uint32_t *)(d_ign + 2 * n_ign));
            uint32_t failed = 0;
            MG_TRY(hipMemcpyAsync(&failed, d_ign + 2 * n_ign, 4, hipMemcpyDeviceToHost, s2));
            MG_TRY(hipStreamSynchronize(s2));
            sc.release(d_ign);
            if (failed)     // Wrap_Around_Back: assert (pos > 0) -- a circular sequence with a reverse frame that has no stop codon (behind the last ignore region)
                return gmg_set_error(GMG_EINVAL, "gmg_find_orfs: a circular sequence has a reverse reading frame without a stop codon (the reference aborts: "
                                                 "Wrap_Around_Back, glimmer_base.cc:2793)");
        } else if (p.orf_bits) {
            hipLaunchKernelGGL(k_mg_find_orfs_bits<true>, dim3(p.ob_grid), dim3(64 * OB_WAVES), 0, s2, a, p.ob_windows, p.ob_win_bases, p.ob_rpw);
        } else if (nr && gmg_opt(GMG_OPT_MG_ORFS_EVENTS)) {
            const uint64_t blocks = (nr + MG_EV_LANES - 1) / MG_EV_LANES;
            if (gmg_opt(GMG_OPT_MG_ORFS_EVENTS) == 1) hipLaunchKernelGGL(k_mg_find_orfs_ev<false>, dim3((unsigned)(blocks < 256 * 128 ? blocks : 256 * 128)), dim3(MG_EV_LANES), 0, s2, a);
            else hipLaunchKernelGGL(k_mg_find_orfs_ev<true>, dim3((unsigned)(blocks < 256 * 128 ? blocks : 256 * 128)), dim3(MG_EV_LANES), 0, s2, a);
        } else if (nr) hipLaunchKernelGGL(k_mg_find_orfs<true>, dim3(grid_for(nr)), dim3(256), 0, s2, a);
        MG_TRY(hipGetLastError());
        tm.lap("find orfs");
        return GMG_OK;
    }

    // the run lengths of the level kernels' walks (they need the reads and the qualities only)
    int build_run_tables(hipStream_t st)
    {
        MG_TRY(sc.alloc(&d_run, (size_t)4 * a.walk_stride));
        a.run_q = d_run; a.run_n = d_run + 2 * a.walk_stride;
        hipLaunchKernelGGL(k_mg_run_tables, dim3(grid_for(2 * nr * 64)), dim3(256), 0, st, a, d_run, d_run + 2 * a.walk_stride);
        MG_TRY(hipGetLastError());
        return GMG_OK;
    }

    // the walk-order rows of the level kernels (running sums, or the values themselves): behind the six-frame table on stream st
    int build_walk_rows(hipStream_t st)
    {
        a.qonly = a.pfx && p.qonly ? 1 : 0;
        MG_TRY(sc.alloc(&d_walk, ((size_t)(a.qonly ? 2 : 6) * a.walk_stride + 8) * sizeof(double)));
        if (a.qonly) {
            // (tried: the same table codon by codon -- a lane on three consecutive steps, ONE scan per class per 192 steps instead of
            // per 64: bit-exact, 23.5 against 22.0 ms per 1M reads with -s: the loads of a lane's three steps no longer coalesce)
            if (a.gene32) hipLaunchKernelGGL((k_mg_walk_prefix<true, true>), dim3(grid_for(2 * nr * 64)), dim3(256), 0, st, a, d_walk + 8);
            else hipLaunchKernelGGL((k_mg_walk_prefix<false, true>), dim3(grid_for(2 * nr * 64)), dim3(256), 0, st, a, d_walk + 8);
        } else if (a.pfx) {
            if (a.gene32) hipLaunchKernelGGL(k_mg_walk_prefix<true>, dim3(grid_for(2 * nr * 64)), dim3(256), 0, st, a, d_walk + 8);
            else hipLaunchKernelGGL(k_mg_walk_prefix<false>, dim3(grid_for(2 * nr * 64)), dim3(256), 0, st, a, d_walk + 8);
        } else
            hipLaunchKernelGGL(k_mg_walk_tables, dim3(grid_for(a.total)), dim3(256), 0, st, a, d_walk + 8);
        a.walk = d_walk + 8;                            // (8 spare entries in front: a call at the table's first entry looks one back)
        MG_TRY(hipGetLastError());
        return GMG_OK;
    }

    // the error branch's walk-order tables, unless the wave / tile kernels build them in LDS
    int err_tables()
    {
        if (res->n_orfs && p.err_mode && p.err_path == 0) {
            // the walk-order tables: the rows (running sums) need the six-frame table and go behind it on the caller's stream; the run
            // lengths need the reads and the qualities only and follow the quality kernel on a stream of their own, beside the ORF scan
            // (second stream), the six-frame kernel and the rows.  Tile by tile (k_mg_err_tile) the rows are built in LDS, tile by tile.
            a.walk_stride = ((a.total + 15) & ~15ull) + 16;
            a.pfx = p.pfx;
            if (a.pfx && !p.err_tile && !p.err_wave) MG_STAGE(build_run_tables(s3));   // running sums + run lengths: the walks visit their events only
            if (!p.err_tile && !p.err_wave) MG_STAGE(build_walk_rows(s));
            MG_TRY(hipGetLastError());
            tm.lap("walk-order tables");
        }
        return GMG_OK;
    }

    // the level kernels' scratch: call arrays, per-ORF aggregates, slot counters
    int alloc_level_scratch()
    {
        a.call_cap = a.total / 2 > 65536 ? a.total / 2 : 65536;
        const uint64_t hinted = (uint64_t)(tl_mg_calls_per_base_hint * 1.15 * (double)a.total) + 65536;
        if (hinted > a.call_cap && hinted <= 8 * a.total + 65536) a.call_cap = hinted;
        if (gmg_opt(GMG_OPT_MG_ERR_CALLS) > 0) a.call_cap = (uint64_t)gmg_opt(GMG_OPT_MG_ERR_CALLS);     // (tests: force the fallback)
        MG_TRY(sc.alloc(&d_calls[0], a.call_cap * sizeof(MgCall)));
        MG_TRY(sc.alloc(&d_calls[1], a.call_cap * sizeof(MgCall)));
        MG_TRY(sc.alloc(&d_agg, no * sizeof(MgOrfAgg)));
        MG_TRY(sc.alloc(&d_fill, no * 4));
        a.calls[0] = d_calls[0]; a.calls[1] = d_calls[1]; a.agg = d_agg; a.fill = d_fill;
        return GMG_OK;
    }

    int alloc_staging(uint64_t entries)
    {
        sc.release(d_st_s);
        sc.release(d_st_e);
        sc.release(d_st_k);
        et_stage_cap = entries;
        MG_TRY(sc.alloc(&d_st_s, entries * sizeof(gmg_start)));
        MG_TRY(sc.alloc(&d_st_e, entries * sizeof(gmg_start_errors)));
        MG_TRY(sc.alloc(&d_st_k, entries * 8));
        return GMG_OK;
    }

    // the error branch's flags and counters, and the scratch of whichever kernel family takes the batch
    int err_scratch()
    {
        if (!(res->n_orfs && p.err_mode && p.err_path == 0)) return GMG_OK;
        MG_TRY(sc.alloc(&d_read_fit, nr ? nr : 1));
        MG_TRY(sc.alloc(&d_err_flag, 256));                 // the flag + the two call counters + six tile counters; tile path: + the number of tiles, the item and staging counters; [32 ..]: the block queues of k_mg_err_wcount (count, write x length class)
        MG_TRY(hipMemsetAsync(d_err_flag, 0, 256, s3));             // (not behind the ORF write pass on the first side stream; both join the caller's below)
        a.read_fit = d_read_fit;
        a.err_flag = d_err_flag;
        a.n_calls = (unsigned long long *)(d_err_flag + 2);
        a.tile_ctr = (unsigned long long *)(d_err_flag + 6);
        d_et_ntiles = d_err_flag + 18;
        d_et_items = (unsigned long long *)(d_err_flag + 20);
        d_et_stage_ctr = (unsigned long long *)(d_err_flag + 22);
        MG_TRY(sc.alloc(&d_acc_bits, (no / 32 + 1) * 4));
        a.acc_bits = d_acc_bits;
        if (p.err_tile) {
            int n_cu = 0;
            MG_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev_id));
            et_grid = (unsigned)(n_cu > 0 ? ET_WG_PER_CU * n_cu : ET_WG_PER_CU * 256);
            // (no more work-groups -- and slabs -- than (tile, strand) pairs: a tile that is closed before it is half full is closed by a
            // read that did not fit, by its 64th read or by its chunk's end)
            const uint64_t tiles_max = a.total / (MG_ET_CAP / 2) + nr / ET_MAXR + a.total / ((uint64_t)ET_CHUNK_TILES * MG_ET_CAP) + 2;
            if (2 * tiles_max < et_grid) et_grid = (unsigned)(2 * tiles_max);
            MG_TRY(sc.alloc(&d_et_tiles, (nr + 1) * sizeof(MgTile)));
            MG_TRY(sc.alloc(&d_et_slabs, (size_t)et_grid * 2 * p.et_qcap * sizeof(MgCall)));
            MG_TRY(sc.alloc(&d_et_em, (size_t)et_grid * p.et_ecap * sizeof(EtEm)));
            // what leaves the tiles: the accepted ORFs' starts (measured: one per 52 bases of 454-like reads) or every start (one per 4)
            uint64_t want = (p.err_acc_only ? a.total / 16 : a.total / 3) + (1u << 20);
            if (gmg_opt(GMG_OPT_MG_ERR_TILE_Q) != 0) want = 64;         // (tests; -1: only this: the first pass finds the arrays too small)
            MG_STAGE(alloc_staging(want));
        } else if (!p.err_wave) MG_STAGE(alloc_level_scratch());
        if (p.err_wave) MG_TRY(sc.alloc(&d_item_flag, 2 * nr + 64));
        return GMG_OK;
    }

    // k_mg_err_wave: as many one-wave work-groups per CU as their LDS shares allow (the grid strides over the (read, strand) pairs)
    hipError_t launch_err_wave(hipStream_t st, bool write)
    {
        const int err_acc_only = p.err_acc_only;
        const uint32_t ew_cap = p.ew_cap, ew_qcap = p.ew_qcap;
        // Length classes, a launch each (a wave's LDS share is sized by its class: more waves per CU for the short reads): up to
        // 384 / 448 / 512 / 704 / EW_MAX_CAP bases.  Both passes on k_mg_err_wcount (breadth first, no walks); mg_err_wave = 2: the stack
        // walker (k_mg_err_wave) for both, 3: the stack walker as the write pass only (cross-checks), up to 512 / ew_cap bases.
        int n_cu = 0;
        hipError_t e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev_id);
        if (e != hipSuccess) return e;
        const long long mode = gmg_opt(GMG_OPT_MG_ERR_WAVE);
        const bool wcount = mode == 1 || (mode == 3 && !write);
        const uint64_t n_blocks = wcount ? (2 * nr + EWC_ITEMS - 1) / EWC_ITEMS : (2 * nr + 63) / 64;
        uint32_t *st_ptr = tm.on && !write ? d_err_flag + 24 : (uint32_t *)nullptr;
        static const uint32_t bounds_c[6] = {0, 384, 448, 512, 704, EW_MAX_CAP}, bounds_w[3] = {0, 512, EW_MAX_CAP};
        const uint32_t *bounds = wcount ? bounds_c : bounds_w;
        const int n_cls = wcount ? 5 : 2;
        // the classes' launches go to streams of their own (forked from st, joined into it): a class's last work-groups run beside the
        // next class's first instead of holding the device for the launch's tail
        MgStreamSet<4, 5> *cs = nullptr;
        if (!tm.on && dev_id >= 0 && dev_id < 16 && !gmg_opt(GMG_OPT_MG_ONE_STREAM)) {
            cs = &tl_mg_streams[dev_id].cls;
            e = cs->need(false, 0);
            if (e == hipSuccess) e = hipEventRecord(cs->ev[4], st);
            if (e != hipSuccess) return e;
        }
        bool used[4] = {false, false, false, false};
        hipStream_t st0 = st;
        for (int cls = 0; cls < n_cls; cls++) {
            if (cs && cls > 0) {
                st = cs->st[cls - 1];
                if (!used[cls - 1]) { e = hipStreamWaitEvent(st, cs->ev[4], 0); if (e != hipSuccess) return e; used[cls - 1] = true; }
            } else st = st0;
            const uint32_t lo = bounds[cls], hi = bounds[cls + 1] < ew_cap ? bounds[cls + 1] : ew_cap;
            if (hi <= lo || reads->max_len <= lo || reads->min_len > hi) continue;
            const uint32_t bytes = wcount ? ewc_layout(bounds[cls + 1], write, a.err_mode == 1).bytes : ew_layout(hi, ew_qcap, write).bytes;
            uint32_t per_cu = (uint32_t)((160u * 1024u) / (bytes + 1024u));
            if (per_cu > 16) per_cu = 16;
            if (per_cu < 1) per_cu = 1;
            uint64_t grid = (uint64_t)(n_cu > 0 ? n_cu : 256) * per_cu * 2;
            if (grid > n_blocks) grid = n_blocks;
            if (grid == 0) continue;
#define MG_EW_LAUNCH(W_, G_, K_) hipLaunchKernelGGL((k_mg_err_wave<W_, G_, K_>), dim3((unsigned)grid), dim3(EW_BLOCK), bytes, st, a, err_acc_only, lo, hi, ew_qcap, d_item_flag, st_ptr)
#define MG_EWC_LAUNCH_I(W_, G_, K_, I_) hipLaunchKernelGGL((k_mg_err_wcount<W_, G_, K_, I_>), dim3((unsigned)grid), dim3(EW_BLOCK), 0, st, a, err_acc_only, lo, hi, d_item_flag, st_ptr, \
                                                                d_err_flag + 32 + (write ? 8 : 0) + cls)
#define MG_EWC_LAUNCH(W_, G_, K_) do { if (a.err_mode == 1) MG_EWC_LAUNCH_I(W_, G_, K_, true); else MG_EWC_LAUNCH_I(W_, G_, K_, false); } while (0)
#define MG_EW_LAUNCH_K(W_, G_) do { if (cls == 0) MG_EW_LAUNCH(W_, G_, 8); else MG_EW_LAUNCH(W_, G_, 15); } while (0)
#define MG_EWC_LAUNCH_K(W_, G_) do { if (cls == 0) MG_EWC_LAUNCH(W_, G_, 6); else if (cls == 1) MG_EWC_LAUNCH(W_, G_, 7); else if (cls == 2) MG_EWC_LAUNCH(W_, G_, 8); else if (cls == 3) MG_EWC_LAUNCH(W_, G_, 11); else MG_EWC_LAUNCH(W_, G_, 15); } while (0)
            if (wcount && write) { if (a.gene32) MG_EWC_LAUNCH_K(true, true); else MG_EWC_LAUNCH_K(true, false); }
            else if (wcount) { if (a.gene32) MG_EWC_LAUNCH_K(false, true); else MG_EWC_LAUNCH_K(false, false); }
            else if (write) { if (a.gene32) MG_EW_LAUNCH_K(true, true); else MG_EW_LAUNCH_K(true, false); }
            else { if (a.gene32) MG_EW_LAUNCH_K(false, true); else MG_EW_LAUNCH_K(false, false); }
#undef MG_EWC_LAUNCH_K
#undef MG_EW_LAUNCH_K
#undef MG_EWC_LAUNCH
#undef MG_EWC_LAUNCH_I
#undef MG_EW_LAUNCH
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        for (int k = 0; k < 4; k++)
            if (used[k]) {
                e = hipEventRecord(cs->ev[k], cs->st[k]);
                if (e == hipSuccess) e = hipStreamWaitEvent(st0, cs->ev[k], 0);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    }

    hipError_t launch_err_tile(hipStream_t st)
    {
        const size_t et_lds = sizeof(EtLds<MG_ET_CAP>);
        const uint32_t et_qcap = p.et_qcap, et_ecap = p.et_ecap;
        const int err_acc_only = p.err_acc_only;
        MgArgs at = a;                                  // the kernel's starts go to the staging arrays
        at.starts = d_st_s; at.errs = d_st_e; at.keys = d_st_k;
#define MG_ET_LAUNCH(G_)                                                                                                         \
        do {                                                                                                                     \
            hipError_t e_ = hipFuncSetAttribute((const void *)k_mg_err_tile<G_, MG_ET_CAP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)et_lds); \
            if (e_ != hipSuccess) return e_;                                                                                     \
            hipLaunchKernelGGL((k_mg_err_tile<G_, MG_ET_CAP>), dim3(et_grid), dim3(ET_BLOCK), et_lds, st, at, d_et_tiles, d_et_ntiles, d_et_items, \
                               d_et_slabs, et_qcap, d_et_em, et_ecap, d_et_stage_ctr, (unsigned long long)et_stage_cap, err_acc_only); \
        } while (0)
        if (a.gene32) MG_ET_LAUNCH(true); else MG_ET_LAUNCH(false);
#undef MG_ET_LAUNCH
        return hipGetLastError();
    }

    // One pass of the error branch over every ORF, the count pass (on st = the joined side stream) or the write pass (the caller's):
    // the wave, tile or level kernels for the reads they take and k_mg_err_flat for the others, or k_mg_err_flat for all
    template <bool WRITE>
    int err_pass(hipStream_t st)
    {
        const int err_acc_only = p.err_acc_only;
        const bool fitted = p.err_path == 0, any_unfit = reads->max_len >= p.err_fit_len();
        if (fitted && p.err_wave) {
            if (WRITE) hipLaunchKernelGGL(k_mg_err_begin, dim3(grid_for(no)), dim3(256), 0, st, a, err_acc_only);
            else {
                if (!wave_reset_done) {
                    MG_TRY(hipMemsetAsync(d_acc_bits, 0, (no / 32 + 1) * 4, st));
                    MG_TRY(hipMemsetAsync(d_item_flag, 0, 2 * nr + 64, st));
                    hipLaunchKernelGGL(k_mg_err_prepare, dim3(grid_for(nr)), dim3(256), 0, st, a, p.err_fit_len());
                }
                wave_reset_done = false;                    // (a repeat of the call starts from zeroed arrays again)
            }
            MG_TRY(launch_err_wave(st, WRITE));
        } else if (fitted && p.err_tile) {
            if (WRITE) hipLaunchKernelGGL(k_et_unstage, dim3(grid_for(no)), dim3(256), 0, st, a, d_st_s, d_st_e, d_st_k, err_acc_only);
            else {
                MG_TRY(hipMemsetAsync(d_acc_bits, 0, (no / 32 + 1) * 4, st));
                const uint64_t chunk = (uint64_t)ET_CHUNK_TILES * MG_ET_CAP, n_chunks = a.total / chunk + 1;
                hipLaunchKernelGGL(k_et_tiles, dim3(grid_for(n_chunks)), dim3(256), 0, st, a, (uint32_t)MG_ET_CAP, (uint32_t)MG_ET_CAP, chunk, n_chunks,
                                   d_et_tiles, d_et_ntiles, d_read_fit);
                MG_TRY(launch_err_tile(st));
            }
        } else if (fitted) {
            const dim3 lvl_grid(256 * 16);
            if (WRITE) hipLaunchKernelGGL(k_mg_err_begin, dim3(grid_for(no)), dim3(256), 0, st, a, err_acc_only);
            else {
                MG_TRY(hipMemsetAsync(d_fill, 0, no * 4, st));
                MG_TRY(hipMemsetAsync(d_acc_bits, 0, (no / 32 + 1) * 4, st));
                hipLaunchKernelGGL(k_mg_err_prepare, dim3(grid_for(nr)), dim3(256), 0, st, a, p.err_fit_len());
            }
#define MG_LEVEL(L_, GRID_) do { if (a.pfx) hipLaunchKernelGGL((k_mg_err_level<WRITE, L_, true>), GRID_, dim3(256), 0, st, a, err_acc_only); \
                                     else hipLaunchKernelGGL((k_mg_err_level<WRITE, L_, false>), GRID_, dim3(256), 0, st, a, err_acc_only); } while (0)
            MG_LEVEL(0, dim3(grid_for(no)));
            MG_LEVEL(1, lvl_grid);
            MG_LEVEL(2, lvl_grid);
#undef MG_LEVEL
            if (!WRITE) hipLaunchKernelGGL(k_mg_err_verdict, dim3(grid_for(no)), dim3(256), 0, st, a, err_acc_only, any_unfit ? 0 : 1);
        }
        if (!fitted || any_unfit) hipLaunchKernelGGL(k_mg_err_flat<WRITE>, dim3(grid_for(no)), dim3(MG_ERR_BLOCK), 0, st, a, err_acc_only, fitted ? 1 : 0);
        return GMG_OK;
    }

    // default mode, the write pass: the fused kernel (running sums + start lists, tile by tile), or k_mg_starts on the sums in HBM
    int default_write_pass()
    {
        const int fused_nw = p.fused_nw, fused_el = p.fused_el;
        const bool fused_nc2 = p.fused_nc2, fused_rest = p.rest;
        if (fused_nw) {
            hipEvent_t side_done = streams ? streams->side.ev[0] : nullptr, cum_done = streams ? streams->side.ev[1] : nullptr;
            const unsigned grid = (unsigned)(2 * a.n_tiles < 64 * 1024 ? 2 * a.n_tiles : 64 * 1024);     // (even: a work-group keeps its strand)
            // the few reads no tile takes (one lane per read, long loops): beside the tile kernel on the side stream, behind their
            // running sums (k_mg_cum, queued on the caller's stream long ago)
            const bool unfit_aside = fused_rest && s2 != s;
            if (unfit_aside) {
                MG_TRY(hipEventRecord(cum_done, s));
                MG_TRY(hipStreamWaitEvent(s2, cum_done, 0));
                hipLaunchKernelGGL(k_mg_starts_unfit, dim3(grid_for(a.n_reads / 16 + 1)), dim3(256), 0, s2, a);
                MG_TRY(hipEventRecord(side_done, s2));
            }
#define MG_LAUNCH_TILE(NW_, G_, EL_) do { if (G_ && a.read_null && NW_ == 2 && EL_ == 8 && fused_nc2) hipLaunchKernelGGL((k_mg_tile_starts<2, G_, 8, G_, 2>), dim3(grid), dim3(128), 0, s, a); \
                                              else if (G_ && a.read_null) hipLaunchKernelGGL((k_mg_tile_starts<NW_, G_, EL_, G_>), dim3(grid), dim3(64 * NW_), 0, s, a); \
                                              else hipLaunchKernelGGL((k_mg_tile_starts<NW_, G_, EL_, false>), dim3(grid), dim3(64 * NW_), 0, s, a); } while (0)
#define MG_LAUNCH_TILE_EL(NW_, G_) do { if (fused_el == 8) MG_LAUNCH_TILE(NW_, G_, 8); else MG_LAUNCH_TILE(NW_, G_, 9); } while (0)
            if (a.gene32) {
                if (fused_nw == 1) MG_LAUNCH_TILE_EL(1, true); else if (fused_nw == 2) MG_LAUNCH_TILE_EL(2, true); else MG_LAUNCH_TILE_EL(4, true);
            } else {
                if (fused_nw == 1) MG_LAUNCH_TILE_EL(1, false); else if (fused_nw == 2) MG_LAUNCH_TILE_EL(2, false); else MG_LAUNCH_TILE_EL(4, false);
            }
#undef MG_LAUNCH_TILE_EL
#undef MG_LAUNCH_TILE
            if (unfit_aside) MG_TRY(hipStreamWaitEvent(s, side_done, 0));
            else if (fused_rest) hipLaunchKernelGGL(k_mg_starts_unfit, dim3(grid_for(a.n_reads / 16 + 1)), dim3(256), 0, s, a);
        } else hipLaunchKernelGGL(k_mg_starts<true>, dim3(grid_for(no)), dim3(256), 0, s, a);
        return GMG_OK;
    }

    // Behind the count pass of the error branch and its scan (which has synchronised the stream): did a staging array, a slab, a
    // stack or a call array overflow?  Then the plan changes, `again` is set and the count pass repeats.
    int count_overflow(int &level_tries, bool &again)
    {
        uint32_t st[32];
        MG_TRY(gmg_copy_wait(st, d_err_flag, 128, hipMemcpyDeviceToHost, s));
        const bool err_tile = p.err_tile, err_wave = p.err_wave;
        if (tm.on && err_tile) fprintf(stderr, "[gmg_mg] k_mg_err_tile: %u tiles (%llu ORFs)\n", st[18], (unsigned long long)no);
        if (tm.on && err_wave)
            fprintf(stderr, "[gmg_mg] k_mg_err_wave: flag %u, deepest stack %u, most ORFs on a strand %u, %u trips and %u calls in %u (read, strand) pairs\n",
                    st[0], st[24], st[25], st[26], st[27], st[28]);
        if (!err_tile && !err_wave && !st[0] && a.total) {   // what this batch needed, for the next call's arrays
            unsigned long long handed[2];
            memcpy(handed, st + 2, 16);
            tl_mg_calls_per_base_hint = (double)(handed[0] > handed[1] ? handed[0] : handed[1]) / (double)a.total;
        }
        if (tm.on && !err_tile && !err_wave) {          // (mg_timing) how many calls the levels handed on
            unsigned long long handed[2];
            memcpy(handed, st + 2, 16);
            fprintf(stderr, "[gmg_mg] calls handed to level 1: %llu, to level 2: %llu (capacity %llu each; %llu ORFs)\n", handed[0], handed[1],
                    (unsigned long long)a.call_cap, (unsigned long long)no);
        }
        if (!st[0]) return GMG_OK;
        again = true;
        if (!(st[0] & 1u) && (st[0] & 2u) && err_tile) {
            // the staging arrays were too small: once more with what the kernel asked for (every batch of ORFs has added its wish)
            unsigned long long asked = 0;
            memcpy(&asked, st + 22, 8);
            MG_STAGE(alloc_staging(asked + 1024));
        } else if (err_tile || err_wave) {
            p.to_level_kernels();
            if (a.q454) { a.q454 = p.q454; MG_STAGE(build_qualities(s2)); }
            if (a.pfx) MG_STAGE(build_run_tables(s2));
            MG_STAGE(build_walk_rows(s2));
            MG_STAGE(alloc_level_scratch());
        } else {
            // once more with arrays of twice what was asked for (level 2 is only partly known when level 1 overflows); if that is
            // not enough either, or does not fit, everything runs on the per-ORF kernel
            unsigned long long asked[2];
            memcpy(asked, st + 2, 16);
            const uint64_t want = 2 * (asked[0] > asked[1] ? asked[0] : asked[1]) + 65536;
            sc.release(d_calls[0]);
            sc.release(d_calls[1]);
            const bool may_grow = level_tries == 0 && want <= 8 * a.total + 65536 && (gmg_opt(GMG_OPT_MG_ERR_CALLS) <= 0 || gmg_opt(GMG_OPT_MG_ERR_CALLS_GROW));
            level_tries++;
            bool grown = false;
            if (may_grow && sc.alloc(&d_calls[0], want * sizeof(MgCall)) == hipSuccess) {
                if (sc.alloc(&d_calls[1], want * sizeof(MgCall)) == hipSuccess) grown = true;
                else sc.release(d_calls[0]);
            }
            if (grown) { a.call_cap = want; a.calls[0] = d_calls[0]; a.calls[1] = d_calls[1]; }
            else {
                p.to_per_orf_kernel();
                a.acc_bits = nullptr;                       // (the verdicts come from the per-ORF kernel from here on: no bitmap)
                if (a.gene32 && !a.fs) {                    // the per-ORF kernel walks the table itself: make it now
                    p.to_fp64_table();
                    const uint64_t fstride = (a.total + 15) & ~15ull;
                    MG_TRY(sc.alloc(&d_fs_own, (size_t)6 * fstride * sizeof(double)));
                    hipLaunchKernelGGL(k_mg_apply_nulls, dim3(grid_for(a.total)), dim3(256), 0, s2, a, d_fs_own, fstride);
                    MG_TRY(hipGetLastError());
                    MG_TRY(hipStreamSynchronize(s2));
                    a.fs = d_fs_own;
                    a.fs_stride = fstride;
                    a.gene32 = nullptr;
                }
            }
        }
        MG_TRY(hipMemsetAsync(d_err_flag, 0, 256, s2));
        MG_TRY(hipMemsetAsync(d_orf_cnt, 0, (no + 1) * 4, s2));
        return GMG_OK;
    }

    // start lists: count pass -> scan -> (error branch) overflow diagnosis and fall-back -> write pass
    int start_lists()
    {
        MG_TRY(sc.alloc(&d_start_off, (no + 1) * 8));
        MG_STAGE(err_scratch());
        hipEvent_t side_done = streams ? streams->side.ev[0] : nullptr;
        // (the wave kernels' zeroed arrays and the reads' fit flags need nothing of the six-frame table: on a side stream, beside the
        // partial-window pass and the ORF write pass -- they sat 0.3 ms between those and the count pass)
        if (no && p.err_mode && p.err_path == 0 && p.err_wave && s3 != s) {      // (the second side stream: the first one is busy with the ORF write pass)
            MG_TRY(hipMemsetAsync(d_acc_bits, 0, (no / 32 + 1) * 4, s3));
            MG_TRY(hipMemsetAsync(d_item_flag, 0, 2 * nr + 64, s3));
            hipLaunchKernelGGL(k_mg_err_prepare, dim3(grid_for(nr)), dim3(256), 0, s3, a, p.err_fit_len());
            MG_TRY(hipGetLastError());
            wave_reset_done = true;
        }
        if (p.err_mode && s2 != s) {                        // the error branch needs the six-frame table from here on: one stream again
            MG_TRY(hipEventRecord(side_done, s2));
            MG_TRY(hipStreamWaitEvent(s, side_done, 0));
            if (s3 != s2) {
                MG_TRY(hipEventRecord(streams->side2.ev[0], s3));
                MG_TRY(hipStreamWaitEvent(s, streams->side2.ev[0], 0));
            }
            s2 = s;
        }
        int level_tries = 0;
        for (int attempt = 0; attempt < 6; attempt++) {
            if (no && p.err_mode) MG_STAGE(err_pass<false>(s2));
            else if (no && !a.count_starts) hipLaunchKernelGGL(k_mg_starts<false>, dim3(grid_for(no)), dim3(256), 0, s2, a);
            MG_TRY(hipGetLastError());
            tm.lap("start lists: count");
            MG_STAGE(mg_scan(d_orf_cnt, d_start_off, no, &res->n_starts, s2));
            if (no && p.err_mode && p.err_path == 0) {
                bool again = false;
                MG_STAGE(count_overflow(level_tries, again));
                if (again) continue;
            }
            if (res->n_starts > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
                return gmg_set_error(GMG_ETOOBIG, "gmg_mg_score_reads: %llu starts in one batch, gmg_mg_orf.start_begin holds %lld: split the batch",
                                     (unsigned long long)res->n_starts, gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
            MG_TRY(sc.alloc(&res->d_starts, (res->n_starts ? res->n_starts : 1) * sizeof(gmg_start)));
            a.start_off = d_start_off;
            a.starts = res->d_starts;
            if (p.err_mode) {
                MG_TRY(sc.alloc(&res->d_errs, (res->n_starts ? res->n_starts : 1) * sizeof(gmg_start_errors)));
                a.errs = res->d_errs;
                if (p.err_path == 0) {
                    MG_TRY(sc.alloc(&d_keys, (res->n_starts ? res->n_starts : 1) * 8));
                    a.keys = d_keys;
                }
            }
            if (s2 != s) {                                  // (mg_scan has synchronised the side stream already; the event keeps
                MG_TRY(hipEventRecord(side_done, s2));      //  the ordering explicit)
                MG_TRY(hipStreamWaitEvent(s, side_done, 0));
            }
            if (no && p.err_mode) MG_STAGE(err_pass<true>(s));
            else if (no) MG_STAGE(default_write_pass());
            MG_TRY(hipGetLastError());
            break;
        }
        return GMG_OK;
    }

    // 4. only what Add_Events_* will see leaves the GPU: two prefix sums over the accepted flags, one gather
    int pack_accepted()
    {
        const int err_mode = p.err_mode, err_path = p.err_path;
        uint32_t *d_keep = nullptr, *d_keep_st = nullptr;
        uint64_t *d_new_orf = nullptr, *d_new_st = nullptr, *d_new_first = nullptr;
        gmg_mg_orf *d_orfs2 = nullptr;
        gmg_start *d_starts2 = nullptr;
        uint64_t n_keep = 0, n_keep_st = 0;
        // Error branch: the write passes put an ORF's starts at the scan of the counts, and a rejected ORF counts 0 -- the start,
        // error and key arrays hold the accepted ORFs' lists alone, in order: packed already.  Only the records move.
        const bool starts_packed = err_mode != 0;
        MG_TRY(sc.alloc(&d_keep, (no + 1) * 4));
        if (!starts_packed) MG_TRY(sc.alloc(&d_keep_st, (no + 1) * 4));
        MG_TRY(sc.alloc(&d_new_orf, (no + 1) * 8));
        if (!starts_packed) MG_TRY(sc.alloc(&d_new_st, (no + 1) * 8));
        MG_TRY(sc.alloc(&d_new_first, (nr + 1) * 8));
        MG_TRY(hipMemsetAsync(d_keep + no, 0, 4, s));
        if (!starts_packed) MG_TRY(hipMemsetAsync(d_keep_st + no, 0, 4, s));
        // (error branch: the bitmap of the accepted ORFs is complete unless everything went to the per-ORF kernel)
        const uint32_t *kept_bits = (err_mode && err_path == 0) ? d_acc_bits : nullptr;
        if (starts_packed && kept_bits && no) {
            const uint64_t n_words = no / 32 + 1;
            uint32_t *d_wc = nullptr, n_keep32 = 0;       // [n_words + 1] set bits per word, then [n_words + 1] their exclusive sums
            MG_TRY(sc.alloc(&d_wc, 2 * (n_words + 4) * 4));
            uint32_t *d_wo = d_wc + ((n_words + 4) & ~3ull);
            hipLaunchKernelGGL(k_mg_keep_words, dim3(grid_for(n_words + 1)), dim3(256), 0, s, kept_bits, n_words, d_wc);
            MG_TRY((gmg_scan_excl<uint32_t, uint32_t>(d_wc, d_wo, n_words + 1, s)));
            MG_TRY(hipMemcpyAsync(&n_keep32, d_wo + n_words, 4, hipMemcpyDeviceToHost, s));
            MG_TRY(hipStreamSynchronize(s));
            n_keep = n_keep32;
            n_keep_st = res->n_starts;
            MG_TRY(sc.alloc(&d_orfs2, (n_keep ? n_keep : 1) * sizeof(gmg_mg_orf)));
            hipLaunchKernelGGL(k_mg_keep_gather_bits, dim3(grid_for(n_words)), dim3(256), 0, s, res->d_orfs, kept_bits, d_wo, n_words, no, d_orfs2);
            hipLaunchKernelGGL(k_mg_keep_reads_bits, dim3(grid_for(nr + 1)), dim3(256), 0, s, res->d_read_orf_off, nr, kept_bits, d_wo, d_new_first);
            MG_TRY(hipGetLastError());
            MG_TRY(hipStreamSynchronize(s));
            sc.release(d_wc);
        } else {
            if (no) hipLaunchKernelGGL(k_mg_keep_counts, dim3(grid_for(no)), dim3(256), 0, s, res->d_orfs, kept_bits, no, d_keep, d_keep_st);
            MG_STAGE(mg_scan(d_keep, d_new_orf, no, &n_keep, s));
            if (starts_packed) n_keep_st = res->n_starts;
            else MG_STAGE(mg_scan(d_keep_st, d_new_st, no, &n_keep_st, s));
            MG_TRY(sc.alloc(&d_orfs2, (n_keep ? n_keep : 1) * sizeof(gmg_mg_orf)));
            if (!starts_packed) MG_TRY(sc.alloc(&d_starts2, (n_keep_st ? n_keep_st : 1) * sizeof(gmg_start)));
            if (no) hipLaunchKernelGGL(k_mg_keep_gather, dim3(grid_for(no)), dim3(256), 0, s, res->d_orfs, kept_bits, res->d_starts, no, d_new_orf,
                                       starts_packed ? (const uint64_t *)nullptr : d_new_st, d_orfs2, d_starts2);
            hipLaunchKernelGGL(k_mg_keep_reads, dim3(grid_for(nr + 1)), dim3(256), 0, s, res->d_read_orf_off, nr, d_new_orf, d_new_first);
            MG_TRY(hipGetLastError());
            MG_TRY(hipStreamSynchronize(s));
        }
        sc.release(d_keep);
        sc.release(d_keep_st);
        sc.release(d_new_orf);
        sc.release(d_new_st);
        sc.release(res->d_orfs);
        sc.release(res->d_read_orf_off);
        if (!starts_packed) { sc.release(res->d_starts); res->d_starts = d_starts2; }     // (else: starts, errors and keys stay where they are)
        res->d_orfs = d_orfs2;
        res->d_read_orf_off = d_new_first;
        res->n_orfs = n_keep;
        res->n_starts = n_keep_st;
        return GMG_OK;
    }

    // 5. error branch: every ORF's slice of the start array into the reference's push order (k_mg_order_starts)
    int push_order()
    {
        if (!(d_keys && res->n_starts)) return GMG_OK;
        const uint64_t ns = res->n_starts, nseg = res->n_orfs;
        gmg_start *d_starts3 = nullptr;
        gmg_start_errors *d_errs3 = nullptr;
        MG_TRY(sc.alloc(&d_starts3, ns * sizeof(gmg_start)));
        MG_TRY(sc.alloc(&d_errs3, ns * sizeof(gmg_start_errors)));
        const uint64_t blocks = (nseg + 3) / 4;
        hipLaunchKernelGGL(k_mg_order_starts, dim3((unsigned)(blocks < 256 * 32 ? blocks : 256 * 32)), dim3(256), 0, s, res->d_orfs, nseg, d_keys, res->d_starts,
                           res->d_errs, d_starts3, d_errs3);
        MG_TRY(hipGetLastError());
        MG_TRY(hipStreamSynchronize(s));
        sc.release(res->d_starts);
        sc.release(res->d_errs);
        res->d_starts = d_starts3;
        res->d_errs = d_errs3;
        tm.lap("start lists: push order");
        return GMG_OK;
    }

    // the call's one wait for the caller's stream; behind it nothing uses the scratch any more
    int finish()
    {
        MG_TRY(hipStreamSynchronize(s));
        tm.lap("start lists");
        if (p.err_wave && res->n_orfs && d_err_flag) {      // did a wave's stack overflow in the WRITE pass?  (the count pass was checked behind its scan)
            uint32_t flag = 0;
            MG_TRY(gmg_copy_wait(&flag, d_err_flag, 4, hipMemcpyDeviceToHost, s));
            if (flag) return MG_RETRY_NO_WAVE;
        }
        return GMG_OK;
    }
};

#undef MG_STAGE
#undef MG_TRY

}                               // namespace

static int mg_run_once(const gmg_model *gene, const gmg_model *nul, const gmg_reads *reads, const gmg_mg_params *prm,
                       double *d_frame_scores, gmg_mg_result **out, void *stream, const bool find_only, const MgGroups *groups)
{
    { int rc_enter = gmg_enter(find_only ? "gmg_find_orfs" : "gmg_mg_score_reads"); if (rc_enter) return rc_enter; }
    { const int rc = mg_check_params(gene, nul, reads, prm, out, find_only); if (rc) return rc; }
    MgTimer tm((hipStream_t)stream);
    int rc;
    {
        MgRun run(gene, nul, reads, prm, d_frame_scores, (hipStream_t)stream, find_only, groups, tm);
        rc = run.run(out);
    }
    if (!rc) tm.lap("free scratch");
    return rc;
}

static int mg_run(const gmg_model *gene, const gmg_model *nul, const gmg_reads *reads, const gmg_mg_params *prm,
                  double *d_frame_scores, gmg_mg_result **out, void *stream, const bool find_only, const MgGroups *groups = nullptr)
{
    int rc = mg_run_once(gene, nul, reads, prm, d_frame_scores, out, stream, find_only, groups);
    if (rc == MG_RETRY_NO_WAVE) {
        tl_mg_no_wave = 1;
        rc = mg_run_once(gene, nul, reads, prm, d_frame_scores, out, stream, find_only, groups);
        tl_mg_no_wave = 0;
    }
    return rc;
}

extern "C" int gmg_mg_score_reads(const gmg_model *gene, const gmg_model *nul, const gmg_reads *reads,
                                  const gmg_mg_params *prm, double *d_frame_scores, gmg_mg_result **out, void *stream)
{
    return mg_run(gene, nul, reads, prm, d_frame_scores, out, stream, false);
}

// glimmer-mg's classification mode: one call for a batch whose reads come in consecutive groups, every group under its own gene
// ICM (the loop over ICM_Sequences, glimmer-mg.cc:361-451), the null model and Ignore_Score_Len per read as in gmg_mg_score_reads
extern "C" int gmg_mg_score_groups(const gmg_mg_group *groups, int n_groups, const gmg_model *nul, const gmg_reads *reads,
                                   const gmg_mg_params *prm, gmg_mg_result **out, void *stream)
{
    if (!groups || n_groups < 1 || !reads || !prm) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_groups: NULL argument");
    if (n_groups >= 1 << 27) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_groups: at most 2^27 - 1 groups per call");
    if (!prm->nulls) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_groups: needs the per-read null models (gmg_mg_params.nulls / read_null)");
    MgGroups g;
    g.n = n_groups;
    uint64_t next = 0;
    for (int k = 0; k < n_groups; k++) {
        if (!groups[k].gene || groups[k].read_begin != next || groups[k].read_end < groups[k].read_begin)
            return gmg_set_error(GMG_EINVAL, "gmg_mg_score_groups: group %d has no model, or the groups are not consecutive read ranges from 0", k);
        if (groups[k].gene->dev.P != 3) return gmg_set_error(GMG_EBADMODEL, "gmg_mg_score_groups: Score_All_Frames needs models of periodicity 3");
        g.models.push_back(groups[k].gene);
        g.read_begin.push_back(next);
        next = groups[k].read_end;
    }
    if (next != reads->n_reads) return gmg_set_error(GMG_EINVAL, "gmg_mg_score_groups: the groups end at read %llu of %llu",
                                                     (unsigned long long)next, (unsigned long long)reads->n_reads);
    g.read_begin.push_back(next);
    return mg_run(groups[0].gene, nul, reads, prm, nullptr, out, stream, false, &g);
}

extern "C" int gmg_find_orfs(const gmg_reads *reads, const gmg_mg_params *prm, gmg_mg_result **out, void *stream)
{
    return mg_run(nullptr, nullptr, reads, prm, nullptr, out, stream, true);
}

extern "C" int gmg_mg_result_info(const gmg_mg_result *r, uint64_t *n_orfs, uint64_t *n_starts)
{
    if (!r) return gmg_set_error(GMG_EINVAL, "gmg_mg_result_info: NULL result");
    if (n_orfs) *n_orfs = r->n_orfs;
    if (n_starts) *n_starts = r->n_starts;
    return GMG_OK;
}

extern "C" int gmg_mg_result_fetch_errors(const gmg_mg_result *r, gmg_start_errors *errs)
{
    { int rc_enter = gmg_enter("gmg_mg_result_fetch_errors"); if (rc_enter) return rc_enter; }
    if (!r || (r->n_starts && !errs)) return gmg_set_error(GMG_EINVAL, "gmg_mg_result_fetch_errors: NULL argument");
    if (!r->n_starts) return GMG_OK;
    if (!r->d_errs) { memset(errs, 0, r->n_starts * sizeof(gmg_start_errors)); return GMG_OK; }
    GMG_HIP(gmg_copy_wait(errs, r->d_errs, r->n_starts * sizeof(gmg_start_errors), hipMemcpyDeviceToHost, r->s));
    return GMG_OK;
}

extern "C" int gmg_mg_result_fetch(const gmg_mg_result *r, gmg_mg_orf *orfs, gmg_start *starts, uint64_t *read_orf_off)
{
    return gmg_mg_result_fetch_on(r, orfs, starts, read_orf_off, nullptr);
}

extern "C" int gmg_mg_result_fetch_on(const gmg_mg_result *r, gmg_mg_orf *orfs, gmg_start *starts, uint64_t *read_orf_off,
                                      void *stream)
{
    { int rc_enter = gmg_enter("gmg_mg_result_fetch_on"); if (rc_enter) return rc_enter; }
    if (!r || (r->n_orfs && !orfs) || (r->n_starts && !starts)) return gmg_set_error(GMG_EINVAL, "gmg_mg_result_fetch: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (r->n_orfs) GMG_HIP(hipMemcpyAsync(orfs, r->d_orfs, r->n_orfs * sizeof(gmg_mg_orf), hipMemcpyDeviceToHost, s));
    if (r->n_starts) GMG_HIP(hipMemcpyAsync(starts, r->d_starts, r->n_starts * sizeof(gmg_start), hipMemcpyDeviceToHost, s));
    if (read_orf_off) GMG_HIP(hipMemcpyAsync(read_orf_off, r->d_read_orf_off, (r->n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    return GMG_OK;
}

#endif
