/* include/hgibbs.h -- C ABI of the MI355X-native BayesRR single-site Gibbs hot path.
 *
 * The reference (medical-genomics-group/hydra) has no plugin/FFI boundary: the
 * sampler is one member function, BayesRRm::runMpiGibbs (src/BayesRRm.cpp:933).
 * This ABI cuts that function at the seam between data load (:1349) and output
 * (:2736): everything N-sized or M-sized lives on the GPU behind an opaque
 * handle, the host keeps only K/G-sized hyper-parameters and the RNG it shares
 * with the device.  Two layers:
 *
 *   hgibbs_*   device operators -- what a maintainer would call from
 *              runMpiGibbs in place of the CPU loops cited per entry point;
 *   hydra_*    the host driver itself (the body of runMpiGibbs restated on top
 *              of hgibbs_*), so that the CLI and language bindings share it.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every call
 * returns 0 on success, non-zero on error (hgibbs_last_error() has the text;
 * like the reference's check_mpi/check_malloc, src/mpi_utils.hpp:19-36, errors
 * are fail-stop for the chain).  One caller thread per handle; calls on one
 * handle are never concurrent.  The library owns all device memory; host
 * buffers are only read/written during the call.  Arrays named *_host are host
 * pointers; nothing in this ABI takes a device pointer.
 */
#ifndef HGIBBS_H
#define HGIBBS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgibbs_ctx* hgibbs_t;

/* MT19937 state shared between host and device (boost::mt19937 of
 * src/distributions_boost.hpp:27; host side drives std::shuffle and the
 * hyper-parameter draws, device side the per-marker draws). */
typedef struct {
    uint32_t x[624];
    uint32_t idx; /* next output position, 624 = twist first */
} hgibbs_rng_state;

const char* hgibbs_last_error(void);
int hgibbs_version(void);

/* ---- lifetime --------------------------------------------------------- */
/* One handle per GPU (one process per GPU in multi-GPU runs). */
int hgibbs_create(int device_id, hgibbs_t* out);
int hgibbs_destroy(hgibbs_t h);

/* ---- individuals sharded across GPUs (replaces the MPI_Allreduce family of
 * src/BayesRRm.cpp:2051,2456,2517-2518 -- SURVEY.md 2.2) ------------------ */
/* rank 0 fills id128 (ncclUniqueId, 128 bytes); the caller broadcasts it by
 * whatever means it has (torch.distributed, MPI, a file) and every rank calls
 * hgibbs_comm_init.  nranks == 1 needs neither call. */
int hgibbs_comm_unique_id(void* id128);
int hgibbs_comm_init(hgibbs_t h, int nranks, int rank, const void* id128);
/* Alternative to RCCL for the rare bulk reductions (load-time counts, per
 * iteration sums): the caller reduces a HOST buffer over its own transport
 * (MPI_Allreduce, gloo ...).  dtype 0 = f64, 1 = u64; returns 0 on success. */
typedef int (*hgibbs_allreduce_fn)(void* user, void* buf_host, size_t count, int dtype);
int hgibbs_comm_init_external(hgibbs_t h, int nranks, int rank, hgibbs_allreduce_fn fn, void* user);
/* In-launch exchange of the per-batch scalars over xGMI: every rank exports a
 * 64-byte IPC handle of its mailbox, the caller gathers the nranks handles
 * (rank order) and every rank imports them.  When imported, hgibbs_sweep sums
 * the ranks' (s1,s2) rows inside the sweep kernel -- each GPU pushes its rows
 * into all peers' mailboxes and adds the nranks contributions in rank order --
 * instead of splitting every batch around an ncclAllReduce launch. */
int hgibbs_p2p_export(hgibbs_t h, void* handle64);
int hgibbs_p2p_import(hgibbs_t h, const void* handles /* nranks * 64 bytes */);

/* ---- data: replaces Data::load_data_from_bed_file + sparse index build
 * (src/data.cpp:671-739, :1224-1290) -------------------------------------- */
/* bed_host: SNP-major packed columns WITHOUT the 3 magic bytes, M columns of
 * stride_in >= ceil(n_total/4) bytes.  keep_host: n_total bytes, 0 drops the
 * individual (NA phenotype, src/data.cpp:1112-1158), NULL keeps all.  Of the
 * kept individuals this rank takes the half-open range [row_begin,row_end)
 * (row_begin % 4 == 0 unless keep_host is given).  n_global = number of kept
 * individuals over all ranks (the N of every formula).
 * Pinned by tests/test_gpu_loader.py: the bits of a column beyond n_total and
 * the bytes beyond ceil(n_total/4) are ignored whatever they hold (PLINK
 * writes 00 there, a called genotype); a shard without a keep list may end
 * anywhere, inside a byte whose other slots are the next rank's rows included;
 * every unused slot of the image (local index >= n_local) is missing, which
 * is what hgibbs_get_bed, the counts and the index lists then show. */
int hgibbs_load_bed(hgibbs_t h, const uint8_t* bed_host, uint64_t stride_in, uint32_t n_total, uint32_t M,
                    const uint8_t* keep_host, uint32_t row_begin, uint32_t row_end, uint32_t n_global);
/* Seeded synthetic genotypes generated directly in HBM (BASELINE.md section 4:
 * g ~ Binomial(2,p_j), p_j ~ U(0.01,0.5), missing calls at missing_rate).
 * Row i of the global matrix depends only on (seed, marker, i), so any
 * sharding yields the same matrix. */
int hgibbs_synth_bed(hgibbs_t h, uint32_t n_global, uint32_t M, uint32_t row_begin, uint32_t row_end,
                     uint64_t seed, double missing_rate);
/* Problem sizes as loaded: N over all ranks, this rank's individuals, markers,
 * first global row of this rank.  Any pointer may be NULL. */
int hgibbs_dims(hgibbs_t h, uint32_t* n_global, uint32_t* n_local, uint32_t* M, uint32_t* row_begin);
/* Copy packed columns [m0, m0+mcount) of this rank's shard back (tests). */
int hgibbs_get_bed(hgibbs_t h, uint32_t m0, uint32_t mcount, uint8_t* out_host, uint64_t out_stride);

/* ---- hydra's sparse representation: replaces Data::load_data_from_sparse_files and the writers behind --bed-to-sparse
 * (layout: src/BayesRRm.cpp:437-770, src/data.cpp:1072-1106, 1224-1290) --------------------------------------------
 * Per marker three lists of 0-based row indices of the file: the rows with genotype 1, with genotype 2, with a missing call
 * (genotype 0 is stored nowhere).  A list of `count` markers is given as the files hold it: start[k] is the ABSOLUTE position of
 * marker k's first entry in the index file (.ss?), len[k] its entries (.sl?), and idx the piece of the index file (.si?) that starts
 * at absolute position idx_base and holds idx_count entries. */
typedef struct {
    const uint64_t* start;
    const uint64_t* len;
    const uint32_t* idx;
    uint64_t idx_base, idx_count;
} hgibbs_sparse_list;
/* Loading: begin, then put in slabs of markers (any cut, any order, each marker once), then end.
 * begin takes hgibbs_load_bed's arguments after the BED pointer, with their meaning and refusals, allocates as it does and fills the
 * image with genotype 0 (padding slots: missing).  Until end succeeds the image is not on the handle: every other call sees a handle
 * without genotypes.
 * put scatters the slab's entries on the device: an entry whose row keep_host drops or that lies outside [row_begin, row_end) is
 * skipped; the order of entries within a list is free.  Refused with a message that names the marker, the row and the fact: a row
 * listed twice for a marker (in one list or in two), an index >= n_total (the smallest such marker and row of the call); and before
 * any device work: a null list, m0 + count > M, a marker put already, start[k] < idx_base, start[k] + len[k] > idx_base + idx_count,
 * len[k] > n_total.  A refused put abandons the load: the handle is as it was before begin.
 * end refuses unless every marker was put; it then publishes the image.  hgibbs_get_bed then returns byte for byte what it returns
 * after hgibbs_load_bed of the equivalent BED with the same keep_host, rows and n_global. */
int hgibbs_sparse_begin(hgibbs_t h, uint32_t n_total, uint32_t M, const uint8_t* keep_host, uint32_t row_begin, uint32_t row_end,
                        uint32_t n_global);
int hgibbs_sparse_put(hgibbs_t h, uint32_t m0, uint32_t count, const hgibbs_sparse_list* ones, const hgibbs_sparse_list* twos,
                      const hgibbs_sparse_list* miss);
int hgibbs_sparse_end(hgibbs_t h);
/* Writing, on one rank (several are refused): counts gives, for markers [m0, m0 + count), the lengths of the three lists over the
 * handle's rows; get writes for each marker in turn the ascending local row indices of genotype 1 into idx1, of genotype 2 into idx2,
 * of missing calls into idxm, each concatenated over the markers and sized by the caller from counts.  Any pointer may be NULL (that
 * output is skipped).  Padding slots are never listed.  The lists are bit-identical for any cut of the markers, any value of the
 * option sparse_piece and any repeat; put back through begin / put / end with keep_host = NULL they reproduce the image. */
int hgibbs_sparse_counts(hgibbs_t h, uint32_t m0, uint32_t count, uint64_t* n1, uint64_t* n2, uint64_t* nm);
int hgibbs_sparse_get(hgibbs_t h, uint32_t m0, uint32_t count, uint32_t* idx1, uint32_t* idx2, uint32_t* idxm);
/* device time in ms of every kernel of the last load (begin .. end, summed; 0 after a refused call) and of the compaction kernels of
 * the last hgibbs_sparse_get (0 after a refused call); host copies are not included.  Either pointer may be NULL. */
int hgibbs_last_sparse_ms(hgibbs_t h, double* put_ms, double* get_ms);

/* a2: per-marker counts and mave/mstd (src/BayesRRm.cpp:1502-1508), counts
 * summed over ranks.  Any output pointer may be NULL. */
int hgibbs_marker_stats(hgibbs_t h, double* mave_host, double* mstd_host, uint64_t* n1_host, uint64_t* n2_host,
                        uint64_t* nmiss_host);

/* ---- residual: eps_host has this rank's row_end-row_begin entries -------- */
int hgibbs_set_residual(hgibbs_t h, const double* eps_host);
int hgibbs_get_residual(hgibbs_t h, double* eps_host);
/* sum and squared norm over ALL ranks (src/BayesRRm.cpp:1677-1678, :2685-2686) */
int hgibbs_reduce_eps(hgibbs_t h, double* sum, double* sqn);
/* eps_i += c (src/BayesRRm.cpp:1675, :1686) */
int hgibbs_add_scalar(hgibbs_t h, double c);
/* eps += x_marker * (-dbeta) ... i.e. the a8 update for one marker on its own
 * (src/BayesRRm.cpp:250-281): eps_i += {v0,v1,v2,0}[g_i] with
 * v0=-(mave*mstd*dbeta), v1=dbeta*(1-mave)*mstd, v2=dbeta*(2-mave)*mstd. */
int hgibbs_update_marker(hgibbs_t h, uint32_t marker, double dbeta);
/* a4 for one marker on its own: num = x_marker' eps (before + beta*(N-1)),
 * summed over ranks (src/BayesRRm.cpp:316-342). */
int hgibbs_dot_marker(hgibbs_t h, uint32_t marker, double* num);

/* ---- fixed-effect covariates (src/BayesRRm.cpp:2648-2681) ---------------- */
/* X_host: this rank's n_local x C covariate values, row-major (what data.X holds
 * for these individuals; hydra expects them standardised: x'x = N-1). */
int hgibbs_set_covariates(hgibbs_t h, const double* X_host, int C);
/* num_f = sum_k X(k,c) * (eps_k + gamma_old * X(k,c)) over all ranks (:2666-2668) */
int hgibbs_cov_dot(hgibbs_t h, int c, double gamma_old, double* num_f);
/* eps_k = eps_k + dgamma * X(k,c), dgamma = gamma_old - gamma_new (:2673-2676) */
int hgibbs_cov_update(hgibbs_t h, int c, double dgamma);

/* ---- model (src/BayesRRm.cpp:1037-1110) --------------------------------- */
/* groups_host[M] in [0,G); cVa/cVaI are G*K row-major with column 0 == 0. */
int hgibbs_set_model(hgibbs_t h, int G, int K, const int32_t* groups_host, const double* cVa_host,
                     const double* cVaI_host);

/* ---- marker effects (replicated on every rank) --------------------------- */
int hgibbs_set_beta(hgibbs_t h, const double* beta_host);
int hgibbs_set_components(hgibbs_t h, const int32_t* components_host); /* restart only */
int hgibbs_get_beta(hgibbs_t h, double* beta_host, int32_t* components_host, double* acum_host);
/* per-group sum of beta^2 in marker order (src/BayesRRm.cpp:2496-2499) */
int hgibbs_beta_sqnorm(hgibbs_t h, double* bsq_host /* G */);

/* ---- the sweep: src/BayesRRm.cpp:1709-2025 (+ :2468-2487) for all M markers
 * in the given order.  order_host[M]; sigmaG_host[G]; estPi_host[G*K];
 * adaV_host[M] (0 = marker frozen out, :1740,:1923-1926).  rng: in = state
 * before the first marker, out = state after the last.  cass_host[G*K] is
 * zeroed then counted (:1697,:1904).  nnz_updates = markers with
 * deltaBeta != 0 (fixes the algorithmic byte count of the sweep). */
int hgibbs_sweep(hgibbs_t h, const int32_t* order_host, double sigmaE, const double* sigmaG_host,
                 const double* estPi_host, const uint8_t* adaV_host, hgibbs_rng_state* rng, int32_t* cass_host,
                 uint64_t* nnz_updates);

/* Tuning knobs of the sweep (not part of the reference's behaviour; every setting gives the same chain up to
 * floating-point rounding, and bit-identical chains on the batch engine with gram = 0).  0 = automatic where noted.
 *   engine          0 auto (default): the resident engine where it applies, else the batch engine; 1 batch engine (one launch
 *                   per batch of markers up to an event); 2 resident engine (ONE launch per sweep; the call fails where it does
 *                   not apply: several ranks without peer mailboxes or more than eight, a
 *                   shard of more than 4096 individuals per compute unit -- 2048 with several ranks or refill = 1 --, G * K > 256).  Setting any option of the batch
 *                   engine below (a batch width, ...) while engine = 0 selects the batch engine.
 *   window          resident engine: columns kept in LDS behind the cursor, a power of two <= 256 (0 auto: 256)
 *   res_cus         resident engine: compute units to use (0 = all; one of them walks the chain, the others stream)
 *   pivots          resident engine: 1 = take the Gram terms of markers whose effect is non-zero at sweep start when a column is
 *                   streamed (their events need no round trip); default 0 (measured slower on MI355X)
 *   refill          resident engine, the streaming workgroups' form: 0 auto (default: 2, unless option pivots is on or the sweep starts
 *                   with a residual beyond the digits' range, |eps| >= 32), 1 = every wave whole columns, three vector instructions per
 *                   genotype (hg_resident.hip.h), 2 = every wave a slice of the individuals, the dots as integer matrix products over
 *                   eps's signed base-256 digits (hg_streamer2.hip.h; needs |eps| < 64: a sweep that meets a larger one fails, error 5)
 *   walker          resident engine: 0 auto (the second where it applies: every marker takes a uniform, <= 4 groups), 1 the
 *                   first walker, 2 the second (hg_walker2.hip.h; the call fails where it does not apply); walker2_ranks: 1 (default) =
 *                   several ranks run the second walker too (without early advances), 0 = they run the first
 *   announce        second walker: 1 (default) = an event that is certain (a marker whose effect is non-zero) is announced before
 *                   its draw, so that its Gram terms travel meanwhile
 *   window_end16    second walker: 1 (default) = the window ends at a multiple of sixteen positions (the second form of the streaming
 *                   workgroups then takes every group of sixteen columns once); 0 = at exactly `window` columns behind the cursor
 *   early_advance   second walker: a walk that runs out of dots moves the window on at once when at least this many positions have
 *                   passed (default 24; 0 = it waits)
 *   bound_slack     second walker, for tests: taken off every threshold of the tabulated bound (default 0).  The bound only ever skips
 *                   exact evaluations, so the chain does not depend on it; from 1000 on every position goes through the exact decision
 *   res_timeout_ms  resident engine: longest wait of any workgroup for another before the sweep is abandoned with an error
 *                   (default 2000); res_deadline_ms: the host's own deadline for the kernel (0 = derived from M, extended while the
 *                   walker's round counter moves)
 *   batch           speculative batch width, 1..256 (0 auto)
 *   cols_per_group  batch columns per workgroup: 2, 4 (default), 8, 16
 *   slices          most tile-group slices per column group, 1..64 (0 auto)
 *   gram            1 (default): continue past predicted events with Gram-corrected dots
 *   max_seg         segments (predicted events) per launch, 1..4 (0 auto by shard size)
 *   ext_limit       longest Gram-corrected extension in columns (default 256)
 *   gram_missing    -1 auto / 0 / 1: take columns with missing calls through the extension (four-term build)
 *   carry           hand the dots of columns behind an unplanned event to the next launch: -1 auto (default: shards of
 *                   400 000 individuals and more), 0 off, 1 on
 *   ahead           columns a launch streams ahead of its batch while its last workgroup draws, 0..256 (default 0: measured
 *                   slower on MI355X; needs carry)
 *   graph           1: replay the launches from a captured HIP graph
 *   ldscore_piece   hgibbs_ld_scores: band rows per piece, 0..2^20 (0 = automatic)
 *   ldmask_piece    hgibbs_ld_mask: band rows per piece, 0..2^20 (0 = automatic; rounded up to a multiple of 16)
 *   grm_piece       hgibbs_grm, hgibbs_grm_rowsums: pairs per piece of rows, 0..2^25 (0 = automatic: 2^25; a row alone may exceed it)
 *   roh_list0       hgibbs_roh: first capacity of the segment list, 0..2^31 (0 = automatic: 2^20; a second run follows an overflow)
 *   ptab_split      hgibbs_pair_tables, hgibbs_epi_scan: ranges of individuals split over workgroups, 0..65535 (0 = automatic)
 *   epi_list0       hgibbs_epi_scan: first capacity of the pair list, 0..2^28 (0 = automatic: 2^20; a second run follows an overflow)
 *   epi_block       hgibbs_epi_scan: list positions a side of a block of the pair space, 0..65536 (0 = automatic: 1024; rounded up to
 *                   a multiple of 32).  A knob for tests of the block scheme, not for tuning: the host waits for the device twice per
 *                   block, which hgibbs_last_epi_ms does not show, so small blocks cost wall time; a block's tables take 72 bytes a pair
 *   rowsums_ranges  hgibbs_row_sums: at most this many ranges of markers split over workgroups, 0..65535 (0 = automatic)
 *   sparse_piece    hgibbs_sparse_get: bytes of index buffers per piece of markers (0 = automatic: a quarter of the free device memory,
 *                   at most 1 GiB; a marker alone may exceed it)
 *   firth_piece     hgibbs_firth_fit: entries of the list per piece (0 = automatic: as many as a quarter of the free device memory holds
 *                   rows of n_local doubles for; a piece holds at least 1 entry and at most 2^24; a negative value is refused)
 *   p2p, force_split, chunk, debug_timing, w_kernel_timing   transport selection and diagnostics */
int hgibbs_set_option(hgibbs_t h, const char* name, int64_t value);
/* The candidate search of the resident engine's second walker, on the host (no device needed; the device code calls the same
 * functions).  masks[i], i < nch <= 4: the candidates of window slots 64 i .. 64 i + 63.  Writes the slots of all candidates in
 * window order from cursor_slot (< 64 nch) on -- upwards, wrapping at 64 nch -- found as the walker finds them: the first, that one
 * cleared, the next.  Returns their number, or -1 (more than cap, bad arguments). */
int hgibbs_walker_search(const uint64_t* masks, uint32_t nch, uint32_t cursor_slot, uint32_t* slots, uint32_t cap);
/* Statistics of the last sweep: launches, markers per launch, device time of
 * the sweep in ms (HIP events on the sweep's stream). */
typedef struct {
    uint64_t launches;        /* launches enqueued (the host enqueues in chunks: a few past the end of the sweep find nothing to do) */
    uint64_t nnz_updates;
    double device_ms;
    double kernel_ms_avg;     /* device_ms / working_launches: average period of the dominant kernel's working launches */
    uint64_t carried_columns; /* batch columns whose dot was handed on by the previous launch instead of being streamed again */
    uint64_t working_launches; /* launches that accepted markers or applied a pending update */
    uint64_t accepted_markers; /* == M after a complete sweep */
    uint64_t streamed_columns; /* batch columns whose dot product was streamed (speculative ones included, carried ones not) */
    uint32_t tiles_per_workgroup_min; /* tile groups of 4096 individuals one workgroup of the sweep kernel streamed per launch: */
    uint32_t tiles_per_workgroup_max; /* > 1 means the loop's next-tile prefetch and cross-tile accumulation ran */
    uint32_t engine;          /* 1 = batch engine (one launch per event batch), 2 = resident engine (one launch per sweep) */
    uint32_t walker;          /* resident engine: 1 = the first walker (the workgroup in lockstep), 2 = the second (one wave walks the chain, hg_walker2.hip.h) */
    double eps_sum_drift;     /* |sum(eps) at sweep end - sum(eps) at sweep start|: s2 of a column without missing calls is taken
                               * once per sweep (src/BayesRRm.cpp:331 re-sums per marker); this is what that assumption costs */
    /* resident engine: rounds of the walker (= working_launches), events (messages that carried an update), rounds that only
     * advanced the window, posterior chunks evaluated, chunks that had to wait for dots streamed behind the last message */
    uint64_t rounds, events, advances, chunks, refolds;
    uint64_t pivots;          /* resident engine: events whose Gram terms were under way before the draw (announced: option announce) or came with the columns (option pivots) */
    uint64_t predicted;       /* resident engine, the census of why rounds end: events at markers whose effect was non-zero at sweep start
                               * (certain to change); events - predicted came unannounced; advances = rounds that ran out of window */
    double shader_mhz;        /* resident engine: s_memtime ticks per microsecond over the sweep (the clock the walker's compute unit held) */
    uint64_t ticks[16];       /* resident engine with option debug_timing: 100 MHz ticks, walker [0] fold [1] collect [2] evaluate
                               * [3] scan + draw [4] message + results + prefetch; streaming workgroup 0: [8] wait [9] update [10] Gram [11] stream */
    uint32_t refill;          /* resident engine: the streaming workgroups' form -- 1 = fused multiply-adds per individual (hg_resident.hip.h),
                               * 2 = integer matrix products over signed base-256 digits of eps (hg_streamer2.hip.h; option refill) */
    uint32_t turned_down;     /* resident engine, second walker: candidates of the tabulated bound that the exact decision found to be no event
                               * (the bound is within about 1e-3 of the function: a handful per sweep; every marker without an event with
                               * option bound_slack >= 1000) */
} hgibbs_sweep_stats;
int hgibbs_last_sweep_stats(hgibbs_t h, hgibbs_sweep_stats* out);
/* measured streaming ceiling of this GPU: device-to-device copy of `bytes` (choose well above the 256 MB
 * Infinity Cache), `reps` times; GB/s counts bytes read + bytes written */
int hgibbs_stream_ceiling(hgibbs_t h, uint64_t bytes, int reps, double* gbps);
/* diagnostic: the 48 accumulated stage-timestamp words (100 MHz ticks) of the sweep kernel's build with option
 * debug_timing = 1 since the last call (which clears them): bench.py's launch anatomy, tools/dbg_times.py */
int hgibbs_debug_times(hgibbs_t h, uint64_t* out48);
/* diagnostic: wall-clock stamps (100 MHz) of the resident engine's last 4096 messages, taken by the build with option
 * debug_timing = 1: 10 rows of 4096 words indexed by message number mod 4096 (`words` <= 10 x 4096 are copied) -- walker: [0] message
 * stored, [1] its Gram terms collected, [2] next message decided, [3] positions it consumed; streaming workgroup 0: [4] message seen
 * (an announced event: the message proper, not its announcement), [5] eps updated, [6] Gram terms sent, [7] refill streamed; rows 8, 9:
 * reserved for experiments (tools/res_anatomy.py reads the first eight) */
int hgibbs_resident_trace(hgibbs_t h, uint64_t* out, uint64_t words);

/* ---- scoring a cohort with posterior effects ------ */
/* For the BED loaded on the handle (this rank's n_local rows, M columns; no collective) and S weight vectors:
 *     out[i*S + s] = sum_j [g_ij not missing] (a[s*M + j] * g_ij + o[s*M + j])
 * with g_ij in {0, 1, 2} the genotype as hgibbs_load_bed reads it; a missing call contributes nothing (mean imputation on the
 * standardised scale when a = beta * mstd, o = -beta * mstd * mave; an allele flip is a = -beta * mstd, o = beta * mstd * (2 - mave)).
 * a, o: S x M row-major host arrays; out: n_local x S row-major.  The sums are exact integer sums of the weights rounded to
 * fixed point, one scale per sample from max_j max(|a_sj|, |o_sj|), so |out - exact| <= 3 M max|weight| 2^-52 and the result
 * does not depend on how the work is split (bit-identical for any S chunking).  Refused: S <= 0, a handle without genotypes,
 * a weight that is not finite.  Options (hgibbs_set_option): score_sp, samples per pass, 2, 4, 8 or 16 (0 = automatic);
 * score_ranges, at most this many ranges of markers split over workgroups (0 = automatic; 1 = every workgroup takes all markers
 * up to 2^21).  The marker-stats counts say which columns have missing calls: when hgibbs_marker_stats has not run, this rank's
 * own counts are taken (no collective). */
int hgibbs_score(hgibbs_t h, int S, const double* a, const double* o, double* out);
/* device time of the last hgibbs_score in ms: every kernel of the call (scales, digits, products, rounding), not the host copies */
int hgibbs_last_score_ms(hgibbs_t h, double* ms);

/* ---- row sums of a function of the genotype */
/* For the BED loaded on the handle and T tables of M x 4 doubles on the host (tab[(t*M + j)*4 + c], table-major),
 *   out[i*T + t] = sum_j tab[(t*M + j)*4 + code_ij]      over the M loaded markers, for this handle's n_local rows
 * where code_ij in {0, 1, 2, 3} is the genotype as the handle stores it: the count of A1 alleles, 3 = missing call.  Padding slots
 * beyond n_local produce no output row.  One pass over the codes on the device.  The contract, which a restatement in integers
 * matches bit for bit:
 *   scale     each table t has one: e_t the smallest integer with max_{j,c} |tab_t[j][c]| < 2^e_t (frexp), E_t = 52 - e_t, and
 *             E_t = 0 for an all-zero table
 *   quantise  q = llrint(ldexp(v, E_t)) (round to nearest, ties to even), written in seven signed base-256 digits
 *   sum       the row's sum is the exact integer sum_j q[t][j][code_ij], turned to f64 ONCE (round to nearest even), times 2^-E_t;
 *             the workgroups' parts meet in 64-bit integer atomic adds, never floating-point ones
 * so |out - exact| <= M max|tab_t| 2^-52 before that one rounding (0.5 2^-E_t per term, 2^-E_t <= 2 max 2^-52); a table whose
 * entries are all 0 or 1 returns the exact count; column t of a call with T tables equals the call with T = 1 and that table; and
 * the result does not depend on any tiling, on the option rowsums_ranges or on repeats.  Refused with a message: a null argument,
 * T outside 1..16, a table entry that is not finite, a handle of several ranks, a handle without genotypes, buffers that do not
 * fit in free device memory (the tables, 16 T bytes per marker of digits for up to 8 tables a pass, 24 T bytes per row), M >= 2^31
 * (the 64-bit sums).  The i32 sums of a digit allow 2^17 blocks of 64 markers per workgroup: longer marker lists are always split
 * into ranges, so that bound refuses nothing.  Option (hgibbs_set_option): rowsums_ranges, at most this many ranges of markers split
 * over workgroups (0 = automatic). */
int hgibbs_row_sums(hgibbs_t h, int T, const double* tab, double* out);
/* device time of the last hgibbs_row_sums in ms: every kernel of the call (scales, digits, products, rounding), not the host
 * copies; 0 after a refused call */
int hgibbs_last_row_sums_ms(hgibbs_t h, double* ms);

/* The exact test of Hardy-Weinberg proportions of Wigginton, Cutler & Abecasis (2005) (host only: no handle, no device).  Given the
 * allele counts of n_het + n_hom_a + n_hom_b genotypes, P(het = k) is proportional to the number of arrangements; the weights are
 * computed by the two-sided recursion outward from the mode and normalised by their sum.  *p = the sum of the probabilities of every
 * feasible k whose probability is <= P(n_het) (1 + 1e-9): the factor is the tie rule, which keeps mirror-image counts from being
 * dropped by a rounding error.  No genotypes: *p = NaN, returns 0.  Refused: a null pointer. */
int hgibbs_hwe_exact(uint32_t n_het, uint32_t n_hom_a, uint32_t n_hom_b, double* p);

/* ---- mean and variance of the scores of marker sets */
/* For the BED on the handle, S weight vectors (a, o: S x M as in hgibbs_score) and nsets marker sets
 * (set r = markers idx[off[r] .. off[r+1]), off[0] = 0, strictly increasing inside a set; sets may overlap, be empty, be scattered):
 *   v_irs       = sum_{j in set r} [g_ij not missing] (a_sj g_ij + o_sj)          (never stored)
 *   mean[r*S+s] = (1/n) sum_i v_irs,   var[r*S+s] = sum_i (v_irs - mean)^2 / (n - 1),   n = n_local
 * Every v_irs is, bit for bit, the value hgibbs_score returns for the same weights with everything outside the set zeroed: the
 * exact integer digit sums of the weights in fixed point and one rounding.  The scale 2^E is therefore one per (set, sample), from
 * max_{j in set} max(|a_sj|, |o_sj|), and |v - exact| <= 3 |set| max_{j in set}|w_sj| 2^-52 per entry -- never more than
 * 3 |set| max|w_s| 2^-52 with the maximum over all of the sample's weights, and as sharp for a set of small effects beside large
 * ones elsewhere.  With d that bound and B the largest |v| of the pair: |mean - exact| <= d + n eps B, and var, computed as
 * (sum v^2 - (sum v)^2 / n) / (n - 1) without centring, is off by at most about 2 n / (n - 1) (2 B d + n eps B^2), eps = 2^-53; with the
 * chain's standardised weights (a = beta mstd, o = -beta mstd mave) the mean is 0 up to rounding and nothing cancels.
 * The sums over i run in one fixed order (a fixed tree inside a block of 256 rows, then the row blocks in ascending order, no
 * floating-point atomics): mean and var are bit-identical across repeats, any chunking of S, any order or chunking of the sets, and
 * every value of the options score_sp and rvar_kb_max.  An empty set gives 0, 0.  var may be NULL.
 * A set of more than rvar_kb_max blocks of 64 markers (option; 0 = default = 32768 blocks, 2^21 markers, the i32 headroom of the
 * digit sums) is scored through hgibbs_score's kernels into an n x samples-per-pass buffer and reduced in the same order.
 * Needs the marker stats (computed here when they are not).  One rank only.  Refused with a message: S <= 0, nsets = 0, n_local < 2,
 * an index >= M, indices not strictly increasing within a set, a weight that is not finite (in a set or not), buffers that do not
 * fit in free device memory, and what one call does not take: 2^24 or more blocks of 64 list entries in all (every set rounded up),
 * more than 65535 x 2^20 pairs of a non-empty set and a block of 256 rows -- pass the sets in several calls. */
int hgibbs_region_var(hgibbs_t h, int S, const double* a, const double* o, uint32_t nsets, const uint64_t* off, const uint32_t* idx,
                      double* mean, double* var);
/* device time of the last hgibbs_region_var in ms: every kernel of the call, not the host copies */
int hgibbs_last_region_var_ms(hgibbs_t h, double* ms);

/* ---- windowed LD of the loaded markers ------------ */
/* For markers j in [m0, m0 + count) and d = 1..W (pairs j, j + d with j + d < M, by index):
 *   r_host[(j - m0) * W + d - 1]        = x_j'x_{j+d} / (N - 1)            (NaN where j + d >= M or either mstd is not finite)
 *   sums_host[((j - m0) * W + d - 1)*4 + t], t = 0..3: the exact integers
 *       G = sum g_j g_q, Bjq = sum g_j [q called], Bqj = sum g_q [j called], D = sum [j called][q called]   (g = 0 at a missing call)
 * with x the chain's standardised genotypes (x = 0 at a missing call), so r is Pearson's r of the allele counts without missing
 * calls and r after mean imputation with them; sums are 0 where j + d >= M.  Either output pointer may be NULL.  Needs the
 * marker stats (hgibbs_marker_stats; computed here when they are not); one rank only (several: error, message); 1 <= W <= 4096;
 * n_local < 2^29.  Every sum is an exact integer, so the results are bit-identical for any m0 / count chunking and any value of the
 * option ld_split (ranges of individuals split over workgroups, 0 = automatic).  Host memory: count * W doubles and 4 count * W
 * int64 at most; the device works in pieces of at most 2^24 pairs. */
int hgibbs_ld(hgibbs_t h, uint32_t m0, uint32_t count, uint32_t W, double* r_host, int64_t* sums_host);
/* device time of the last hgibbs_ld in ms: every kernel of the call (zeroing, products, final formula), not the host copies */
int hgibbs_last_ld_ms(hgibbs_t h, double* ms);

/* ---- LD scores of the loaded markers -------------- */
/* l2[j*C + c] = a_jc + sum_{q != j in j's window} a_qc t_jq over the M loaded markers (marker-major), where
 *   window   a pair (j, q), j < q, is in the window iff q - j <= ahead[j]; it counts for both of its markers.  ahead: M entries with
 *            ahead[j] <= W and j + ahead[j] < M, or NULL for min(W, M - 1 - j)
 *   a_qc     bit c of annot[q] (binary annotations), 1 <= C <= 64 and no bit at or above C; annot = NULL means C = 1 with every marker
 *   t_jq     r^2, or with adjust != 0 the estimator r^2 - (1 - r^2) / (N - 2), N = n_global (N >= 3); r is exactly hgibbs_ld's r
 * A marker whose mstd is not finite contributes to nobody and its own row is NaN in every column.  The band never leaves the device:
 * the four integer sums of a piece of band rows (hgibbs_ld's products, at most 2^24 pairs) are reduced there, forwards and backwards,
 * into an M x C accumulator of signed 64-bit fixed point, llrint(t 2^44) per pair with integer adds, converted once at the end.  So
 * the result is bit-identical for any value of the options ldscore_piece (band rows per piece, 0 = automatic, rounded up to a multiple
 * of 16, at most 2^20) and ld_split and for any repeat, and column c of a call with C columns equals the call with C = 1 and annot
 * reduced to bit c.  |l2 - exact| <= (terms of the marker's window) x 2^-45 beyond the rounding of r.  One rank only; 1 <= W <= 4096;
 * n_local < 2^29; refused when the accumulator and a piece's sums do not fit in free device memory. */
int hgibbs_ld_scores(hgibbs_t h, uint32_t W, const uint32_t* ahead, uint32_t C, const uint64_t* annot, int adjust, double* l2);
/* device time of the last hgibbs_ld_scores in ms: the products (zeroing and hgibbs_ld's product kernel, every piece) and the reduce
 * (the reduction kernel of every piece, zeroing the accumulator and the final conversion); not the host copies */
int hgibbs_last_ld_scores_ms(hgibbs_t h, double* products_ms, double* reduce_ms);

/* ---- LD masks and the greedy selection on them ----- */
/* One bit per pair of the band of the M loaded markers, forwards and backwards:
 *   window   exactly that of hgibbs_ld_scores: a pair (j, q), j < q, is in the window iff q - j <= ahead[j].  ahead: M entries with
 *            ahead[j] <= W and j + ahead[j] < M (refused otherwise), or NULL for min(W, M - 1 - j)
 *   passes   a pair passes iff it is in the window, r is not NaN, and r * r >= t.  r is exactly hgibbs_ld's r, so both markers have a
 *            finite mstd; the comparison is done on the f64 product
 *   masks    wpr = (W + 63) / 64 words per marker.
 *            fwd[j*wpr + (d-1)/64] bit (d-1)%64 is set iff pair (j, j + d) passes;
 *            bwd[q*wpr + (d-1)/64] bit (d-1)%64 is set iff q >= d and pair (q - d, q) passes.
 *            Every other bit is 0, including the bits of offsets above W in a row's last word.  bwd may be NULL.
 *   npass    may be NULL: the number of passing pairs
 * t must be finite and >= 0 (refused otherwise, with a message); t = 0 gives every in-window pair with a finite r.  The band never
 * leaves the device: the four integer sums of a piece of band rows (hgibbs_ld's products, at most 2^24 pairs) are reduced there to the
 * two masks, with plain stores forwards and 64-bit atomic ORs backwards.  So the result is bit-identical for any value of the options
 * ldmask_piece (band rows per piece, 0 = automatic, rounded up to a multiple of 16, at most 2^20) and ld_split and for any repeat.
 * One rank only; 1 <= W <= 4096; n_local < 2^29; a handle without genotypes and a null fwd are refused, and so is a call whose two
 * M x wpr x 8-byte masks and a piece's sums do not fit in free device memory. */
int hgibbs_ld_mask(hgibbs_t h, uint32_t W, const uint32_t* ahead, double t, uint64_t* fwd, uint64_t* bwd, uint64_t* npass);
/* device time of the last hgibbs_ld_mask (or hgibbs_ld_clump) in ms: the products (zeroing the sums and hgibbs_ld's product kernel, every
 * piece) and the reduce (zeroing the masks and the reduction kernel of every piece); not the host copies */
int hgibbs_last_ld_mask_ms(hgibbs_t h, double* products_ms, double* reduce_ms);
/* The greedy selection on two masks in hgibbs_ld_mask's layout (host only: no handle, no device).  order holds norder distinct marker
 * indices below M, the participating markers in descending priority (a duplicate or an index >= M is refused by name); may_lead has M
 * bytes, or is NULL for "all may".  owner[M] starts at -1 everywhere; then for k = 0 .. norder - 1, with v = order[k]:
 *   if owner[v] != -1, continue; if v may not lead, continue;
 *   otherwise owner[v] = v, and every participating q whose pair with v passes and whose owner is -1 gets owner[q] = v.  A pair with v
 *   passes when its bit is set in v's forward or backward row.
 * This is PLINK's clump walk: a participating marker that may not lead and is never claimed stays -1, and so does every marker that
 * does not participate.  Refused: W outside 1..4096, M = 0 or M >= 2^31, a null fwd, bwd or owner, a null order with norder > 0. */
int hgibbs_ld_greedy(uint32_t M, uint32_t W, const uint64_t* fwd, const uint64_t* bwd, const uint32_t* order, uint32_t norder,
                     const uint8_t* may_lead, int32_t* owner);
/* hgibbs_ld_mask into internal host buffers, then hgibbs_ld_greedy on them: owner is by definition what the two calls give, it refuses
 * what either refuses, and hgibbs_last_ld_mask_ms stays valid after it.  npass may be NULL. */
int hgibbs_ld_clump(hgibbs_t h, uint32_t W, const uint32_t* ahead, double t, const uint32_t* order, uint32_t norder,
                    const uint8_t* may_lead, int32_t* owner, uint64_t* npass);

/* ---- the Gibbs sweep from summary statistics and the panel's LD band ---- */
/* The chain's step with c_j = x_j'eps kept per marker instead of the residual per individual.  Inputs: n_eff; xty[j] = b_j = x_j'y
 * for a y with y'y = n_eff - 1; and the symmetric band B_jk = (n_eff - 1) r_jk, r exactly hgibbs_ld's r of the loaded panel, for the pairs
 * of hgibbs_ld_scores' window (ahead: M entries with ahead[j] <= W and j + ahead[j] < M, or NULL for min(W, M - 1 - j)); pairs outside the
 * window count as 0, and so does every pair with a marker whose mstd is not finite (such a marker is never adaptive either).
 *   begin    builds the band once on the device from the loaded image (M x W doubles, the `ahead` half only; it never crosses the bus),
 *            sets c = xty and every effect, component and acum to 0.  n_eff need not be the panel's row count: r comes from the panel,
 *            the scale from the summary statistics.  Refused by name: a null handle, no genotypes, several ranks, W outside 1..4096,
 *            an `ahead` entry out of range, n_eff not finite or below 2, a null or non-finite xty, buffers that do not fit in free
 *            device memory.  A second call replaces the state of the first.
 *   sweep    hgibbs_sweep's signature and meaning, on the model of hgibbs_set_model.  Per marker j in the given order:
 *            num = c_j + (n_eff - 1) beta_j; the reference's decision and draw; with delta = beta_old - beta_new != 0,
 *            c_k += delta B_jk over j's window on both sides and c_j += delta (n_eff - 1).  The effects, components and acum live where
 *            hgibbs_get_beta, hgibbs_set_beta, hgibbs_set_components and hgibbs_beta_sqnorm read and write them (hgibbs_set_beta changes
 *            the effects alone: c stays as it is).  One launch, one workgroup; two runs from the same state give the same bits.
 *   state    c (M doubles, may be NULL) and sum_j beta_j b_j, sum_j beta_j c_j (either may be NULL), each summed in marker order over the
 *            non-zero effects on the device: a fixed order, bit-reproducible.
 *   band_get the band rows [m0, m0 + count): count x W doubles, out[(j - m0) W + d - 1] = B_{j, j + d}, 0 for d > ahead[j].
 *   end      frees the state (hgibbs_destroy does too).
 *   last_ss_ms   device time of hgibbs_ss_begin's band (zeroing, products, scaling) and of the last hgibbs_ss_sweep's kernel. */
int hgibbs_ss_begin(hgibbs_t h, double n_eff, uint32_t W, const uint32_t* ahead /* M or NULL */, const double* xty /* M */);
int hgibbs_ss_sweep(hgibbs_t h, const int32_t* order_host, double sigmaE, const double* sigmaG_host, const double* estPi_host,
                    const uint8_t* adaV_host, hgibbs_rng_state* rng, int32_t* cass_host, uint64_t* nnz_updates);
int hgibbs_ss_state(hgibbs_t h, double* c_out, double* beta_b, double* beta_c);
int hgibbs_ss_band_get(hgibbs_t h, uint32_t m0, uint32_t count, double* out);
int hgibbs_ss_end(hgibbs_t h);
int hgibbs_last_ss_ms(hgibbs_t h, double* band_ms, double* sweep_ms);
/* The same sweep on host arrays (host only: no handle, no device), the yardstick of the device engine: band is M x W in
 * hgibbs_ss_band_get's layout (entries beyond ahead[j] are not read), c, beta, components and acum are the state (M each, updated in
 * place), G, K, groups (M, or NULL for one group), cVa and cVaI are hgibbs_set_model's, the rest is hgibbs_ss_sweep's.  With a band that
 * covers every pair and b = X'y this is the individual-level sweep: c_j stays x_j'eps. */
int hgibbs_ss_sweep_host(uint32_t M, double n_eff, uint32_t W, const uint32_t* ahead, const double* band, double* c, double* beta,
                         int32_t* components, double* acum, int G, int K, const int32_t* groups, const double* cVa, const double* cVaI,
                         const int32_t* order, double sigmaE, const double* sigmaG, const double* estPi, const uint8_t* adaV,
                         hgibbs_rng_state* rng, int32_t* cass, uint64_t* nnz_updates);

/* ---- independent LD blocks swept at the same time ---- */
/* A cut lies before marker j (1 <= j < M) iff no window crosses that place: max over k < j of (k + ahead[k]) < j.  Between two cuts
 * the band is a block of its own, and given mu, sigmaE, sigmaG and pi the effects of different blocks are conditionally independent:
 * sweeping them at the same time, each from a generator of its own, is an exact Gibbs sampler of the same posterior.  It draws another
 * realisation than hgibbs_ss_sweep does from one generator, so no parity with the single stream (or the reference) is claimed.
 *   partition      (host only) walks the blocks in marker order into intervals: an interval closes as soon as it holds at least
 *                  ceil(M / S_max) markers, the remainder is the last.  bounds (room for S_max + 1) gets 0 = bounds[0] < ... < bounds[S] = M,
 *                  1 <= S <= S_max <= 1024; deterministic.
 *   sweep_streams  hgibbs_ss_sweep with S generators: one launch, one workgroup per interval.  Interval s sweeps its own markers in the
 *                  order `order_host` lists them, with rngs[s] (in and out).  cass and nnz_updates are the sums over the intervals.
 *                  Refused by name beyond hgibbs_ss_sweep's refusals: S outside 1..1024, bounds that do not run from 0 to M strictly
 *                  ascending, an interior bound that is not a cut (with the marker whose window crosses it), an idx above 624 in any
 *                  state, an order that is no permutation.  With S = 1 it gives hgibbs_ss_sweep's bits.  hgibbs_last_ss_ms reports its
 *                  kernel as it does hgibbs_ss_sweep's.
 *   sweep_streams_host  (host only) the same on host arrays, interval after interval: what the device is held to. */
int hgibbs_ss_partition(uint32_t M, const uint32_t* ahead, uint32_t S_max, uint32_t* bounds /* S_max + 1 */, uint32_t* S);
int hgibbs_ss_sweep_streams(hgibbs_t h, const int32_t* order_host, double sigmaE, const double* sigmaG_host, const double* estPi_host,
                            const uint8_t* adaV_host, uint32_t S, const uint32_t* bounds /* S + 1 */, hgibbs_rng_state* rngs /* S */,
                            int32_t* cass_host, uint64_t* nnz_updates);
int hgibbs_ss_sweep_streams_host(uint32_t M, double n_eff, uint32_t W, const uint32_t* ahead, const double* band, double* c, double* beta,
                                 int32_t* components, double* acum, int G, int K, const int32_t* groups, const double* cVa, const double* cVaI,
                                 const int32_t* order, double sigmaE, const double* sigmaG, const double* estPi, const uint8_t* adaV, uint32_t S,
                                 const uint32_t* bounds, hgibbs_rng_state* rngs, int32_t* cass, uint64_t* nnz_updates);

/* ---- several chains on one band ---- */
/* R replicas of the chain's state beside the handle's own, between hgibbs_ss_begin and hgibbs_ss_end.  A replica has its own c, effects,
 * components, acum, order, mask, mixture tables, cass and generator(s); the band, its window, xty, the groups and the model are the
 * handle's.  The handle's own chain (what hgibbs_ss_sweep, hgibbs_get_beta, hgibbs_ss_state and hgibbs_beta_sqnorm use) is no replica:
 * no call below reads or writes it, and no call above reads or writes a replica.
 *   replicas        R in 1..64 replicas with c = xty and every effect, component and acum 0; a second call replaces the first's.
 *                   Refused by name: no ss state, R out of range, memory that does not fit (with R and the bytes).
 *   sweep_replicas  ONE launch, S x R workgroups: workgroup (s, r) sweeps interval s of replica r.  orders R x M, sigmaE R, sigmaG
 *                   R x G, estPi R x G x K, adaV R x M (a chain's mask is its own: a group can freeze out in one chain alone),
 *                   bounds S + 1 (NULL with S = 1: {0, M}), rngs R x S (replica-major, in and out), cass R x G x K, nnz_updates R
 *                   (or NULL).  Replica r's outcome -- effects, components, acum, c, cass, nnz, every generator's words and index --
 *                   is bit for bit what hgibbs_ss_sweep_streams gives from the same state and arguments on the handle's own chain,
 *                   and with S = 1 what hgibbs_ss_sweep gives.  Refused as hgibbs_ss_sweep_streams refuses, with the replica's
 *                   number; and by name: replicas not allocated, an R other than the allocated one.  hgibbs_last_ss_ms reports it.
 *   replica_sums    one launch, a wave per replica: sb[r] = sum beta_j b_j, sc[r] = sum beta_j c_j (hgibbs_ss_state's order and bits)
 *                   and bsq[r G + g] (hgibbs_beta_sqnorm's); any pointer may be NULL.  At most 8192 groups.
 *   replica_get     replica r's effects, components, acum and c (any pointer may be NULL)
 *   replica_set_beta  replica r's effects alone: c stays as it is, as with hgibbs_set_beta */
int hgibbs_ss_replicas(hgibbs_t h, uint32_t R);
int hgibbs_ss_sweep_replicas(hgibbs_t h, uint32_t R, const int32_t* orders, const double* sigmaE, const double* sigmaG, const double* estPi,
                             const uint8_t* adaV, uint32_t S, const uint32_t* bounds, hgibbs_rng_state* rngs, int32_t* cass_host,
                             uint64_t* nnz_updates);
int hgibbs_ss_replica_sums(hgibbs_t h, double* sb /* R */, double* sc /* R */, double* bsq /* R x G */);
int hgibbs_ss_replica_get(hgibbs_t h, uint32_t r, double* beta, int32_t* comp, double* acum, double* c);
int hgibbs_ss_replica_set_beta(hgibbs_t h, uint32_t r, const double* beta);

/* ---- the per-marker posterior table, accumulated on the device ---- */
/* Per marker over T planned records of every chain: the posterior mean and sd of the effect, the inclusion probability, the draws per
 * component, and split-R^ over the 2 C half-chains (hgibbs_mcmc_diag's split and formulas), folded where the chains' state lies: no
 * record crosses the bus.  C = R chains for R >= 1 (the R allocated replicas), C = 1 for R = 0 (the handle's own chain: what
 * hgibbs_ss_sweep and hgibbs_ss_sweep_streams write).  A record is the chains' effects and components as they stand at the call.
 *   post_begin  allocates and zeroes the accumulators: the pooled Welford pair (mean, m2) per marker, the pair of every half-chain
 *               (C x 2 x M), the counts K x M.  T is planned in advance because the split needs it: with n = T / 2, record t (0-based,
 *               the number of adds so far) lies in half 0 if t < n and in half 1 if t >= T - n; an odd T leaves the middle record in
 *               neither.  A second call replaces the first's state.  Refused by name: no ss state; R >= 1 without replicas, or another R
 *               than the allocated one; T < 4; R T >= 2^32; no model set (K is not known); memory that does not fit (with R, T and the
 *               bytes).  While the state is open hgibbs_ss_replicas and hgibbs_set_model are refused; hgibbs_ss_end frees it too.
 *   post_add    ONE launch, a thread per marker, the chains in order r = 0 .. C - 1: a Welford step d = x - mean; mean = mean + d / q;
 *               m2 = m2 + d (x - mean) into the pooled pair with q = t C + r + 1, the same step into chain r's half-chain pair with the
 *               count inside the half where t lies in one, and cnt[comp][j] += 1.  Only correctly rounded f64 + - x / in a fixed order:
 *               the accumulators repeat bit for bit.  Reads the chains' state and writes none of it.  Refused: before post_begin; beyond
 *               T; a component outside [0, K) (with the chain and the marker; the accumulators are dropped).
 *   post_get    after exactly T adds: mean = the pooled mean, sd = sqrt(m2 / (C T - 1)), pip = (C T - cnt[0]) / (C T), cnt (K x M,
 *               cnt[k M + j]), rhat (NaN where no half-chain moves: !(W > 0)); M each but cnt, any pointer may be NULL.
 *   post_raw    after exactly T adds: the pair (mean, m2) of half `half` (0, 1) of chain r in [0, C), or with r = C and half = 0 the pooled
 *               pair; M doubles each, either may be NULL.  Refused: r or half out of range.
 *   post_end    frees the accumulators.
 *   last_ss_post_ms  device time of every post_add kernel since post_begin (their sum) and of post_get's kernel; 0 without a state. */
int hgibbs_ss_post_begin(hgibbs_t h, uint32_t R, uint32_t T);
int hgibbs_ss_post_add(hgibbs_t h);
int hgibbs_ss_post_get(hgibbs_t h, double* mean, double* sd, double* pip, uint32_t* cnt /* K x M */, double* rhat);
int hgibbs_ss_post_raw(hgibbs_t h, uint32_t r, uint32_t half, double* hmean, double* hm2);
int hgibbs_ss_post_end(hgibbs_t h);
int hgibbs_last_ss_post_ms(hgibbs_t h, double* add_ms, double* final_ms);

/* ---- local credible sets from the chains' inclusion history, kept on the device ---- */
/* One bit per marker and record, kept where the chains' state lies; counts, candidate sets and their posterior existence probabilities
 * (PEP) come from it with bit operations: exact integers, no record over the bus.  Everything below is integer.
 *   history   a state is opened for C chains x T planned records, NREC = C T < 2^32.  Record q = t C + r (t adds so far, chain r);
 *             marker j's bit q is 1 iff it is in the model in that record.  hist[(q / 64) M + j] bit q % 64; NW = (NREC + 63) / 64 words
 *             per marker; every bit at or above the records added so far is 0.  cnt[j] = the popcount of marker j's words.
 *   cs_begin  allocates and zeroes the history.  A second call replaces the first's state; hgibbs_destroy frees it; hgibbs_ss_end does
 *             not (the state does not depend on the ss state).  Refused by name: a null handle or no genotypes, several ranks, C = 0,
 *             T = 0, C T >= 2^32, memory that does not fit (with M, NREC and the bytes).
 *   adds      cs_add_flags (flags: C x M bytes, non-zero = in the model) and ss_cs_add (chain r's component != 0; R as
 *             hgibbs_ss_post_begin's: 0 the handle's own ss chain, >= 1 the replicas) each add ONE record of every chain: one launch, a
 *             thread per marker, plain loads and stores.  ss_cs_add reads the chains' state and writes none of it.  Refused by name:
 *             before cs_begin, beyond T, null flags; ss_cs_add without ss state, R >= 1 without replicas or another R than allocated,
 *             max(R, 1) != C.
 *   cs_counts, cs_history, cs_sets  may be called after any number of adds and describe the records added so far (NREC = t C).
 *             cs_history always copies the whole NW x M words.
 *   cs_sets   masks fwd, bwd in hgibbs_ld_mask's layout for window width W (wpr = (W + 63) / 64): marker v + d is a friend of lead v iff
 *             bit d - 1 of v's forward row is set, marker v - d iff bit d - 1 of its backward row is; bits of offsets above W and of
 *             markers that do not exist are ignored.  Per lead v: members = [v], sum = cnt[v]; while sum < need: with max_size members
 *             the set fails with status 2 (cap); otherwise the friend not yet taken with the largest cnt > 0, ties to the smallest
 *             index, is appended and its cnt added; if there is none the set fails with status 1 (short).  On success (status 0) size =
 *             the number of members and pep = the popcount of the OR of the members' history words.  A failed candidate reports size 0,
 *             pep 0 and the sum it reached.  members is nlead x max_size; the slots from `size` on hold 0xFFFFFFFF (all of a failed
 *             candidate's).  The results do not depend on the order of the leads or on how they are split over calls.  Refused by
 *             name: no open state, W outside 1..4096, null masks, a lead >= M, a lead listed twice, need = 0, max_size outside 1..256.
 *   last_cs_ms  the sum of all add kernels since cs_begin, the last counts kernel, the last sets kernel (the latter two 0 after a
 *             refused call of theirs); all 0 without a state. */
int hgibbs_cs_begin(hgibbs_t h, uint32_t C, uint32_t T);
int hgibbs_cs_add_flags(hgibbs_t h, const uint8_t* flags /* C x M, non-zero = in the model */);
int hgibbs_ss_cs_add(hgibbs_t h, uint32_t R);
int hgibbs_cs_counts(hgibbs_t h, uint32_t* cnt /* M */);
int hgibbs_cs_history(hgibbs_t h, uint64_t* out /* NW x M */);
int hgibbs_cs_sets(hgibbs_t h, uint32_t W, const uint64_t* fwd, const uint64_t* bwd, uint32_t nlead, const uint32_t* leads,
                   uint32_t need, uint32_t max_size, uint32_t* status, uint32_t* size, uint64_t* sum, uint32_t* pep,
                   uint32_t* members /* nlead x max_size */);
int hgibbs_cs_end(hgibbs_t h);
int hgibbs_last_cs_ms(hgibbs_t h, double* add_ms, double* counts_ms, double* sets_ms);
/* The walk over hgibbs_cs_sets' candidates (host only: no handle, no device): by descending lead_cnt, ties by ascending lead index
 * (std::stable_sort); a candidate is accepted iff its status is 0, its pep >= min_pep and none of its members belongs to a set accepted
 * before it.  taken[0 .. *ntaken) are the accepted candidates' positions in the order taken: the sets are disjoint.  Refused by name:
 * null pointers, max_size outside 1..256, a size above max_size, a member >= M inside a size. */
int hgibbs_cs_select(uint32_t M, uint32_t nlead, const uint32_t* leads, const uint32_t* lead_cnt, const uint32_t* status,
                     const uint32_t* size, const uint32_t* pep, const uint32_t* members, uint32_t max_size, uint32_t min_pep,
                     uint32_t* taken /* nlead */, uint32_t* ntaken);

/* Convergence of R chains of one scalar (host only): x is R x T, chain-major.  mean and sd over all R T draws; rhat: split-R^ (BDA3
 * section 11.4: every chain halved, an odd T drops the middle draw; no rank normalisation); ess: from the same 2 R half-chains'
 * combined autocovariances, truncated by Geyer's initial monotone positive sequence (Stan reference manual), at most
 * 2 R n log10(2 R n) with n = T / 2.  No within-chain variance at all: rhat and ess are NaN.  Any output may be NULL.  Refused by name:
 * null x, R = 0, T < 4.  Every sum runs in index order. */
int hgibbs_mcmc_diag(uint32_t R, uint32_t T, const double* x, double* mean, double* sd, double* rhat, double* ess);

/* ---- dots of the loaded markers against dense vectors */
/* For markers j in [m0, m0 + count) of the loaded BED and K vectors u_k over this rank's n_local individuals:
 *   out[(j - m0)*K + k]           = x_j'u_k = mstd_j (P_jk - mave_j Q_jk)      (NaN where mstd_j is not finite)
 *   raw[((j - m0)*K + k)*2 + 0/1] = P_jk = sum_{i called} g_ij u_ik,  Q_jk = sum_{i called} u_ik
 * U: K x n_local row-major (U[k*n_local + i]).  raw may be NULL.
 * x is the chain's standardised genotype (x = 0 at a missing call), g in {0, 1, 2} the genotype as hgibbs_load_bed reads it.  Each
 * vector gets one scale, E_k = 52 - e_k with max_i |u_ik| < 2^e_k (E_k = 0 for an all-zero vector), and q = llrint(u 2^E_k); P and Q
 * are the exact integer sums of the q's, each rounded to f64 once (times 2^-E_k).  The only error is the rounding of u:
 * |P - sum g u| <= n 2^-E_k <= 2 n max|u_k| 2^-52 and |Q - sum u| <= n max|u_k| 2^-52 before that one rounding, so the results are
 * bit-identical for any m0 / count chunking, any value of the option mdots_split (ranges of individuals split over workgroups,
 * 0 = automatic) and any repeat.  Needs the marker stats (computed here when they are not).  Refused: K <= 0 or K > 32 (the LDS
 * staging takes four tiles of two vectors a pass, at most four passes), a non-finite entry of U, m0 + count > M, a handle without
 * genotypes, several ranks, n_local >= 2^29. */
int hgibbs_marker_dots(hgibbs_t h, uint32_t m0, uint32_t count, int K, const double* U, double* out, double* raw);
int hgibbs_last_marker_dots_ms(hgibbs_t h, double* ms);   /* every kernel of the last call, not the host copies */

/* ---- sums of dense vectors over the rows of each genotype code, per marker */
/* For markers j in [m0, m0 + count) of the loaded BED and K vectors u_k over this rank's n_local individuals (U as
 * hgibbs_marker_dots takes it: U[k*n_local + i]):
 *   out[((j - m0)*K + k)*4 + c] = S_jkc = sum_{i : code_ij = c} u_ik,   c = 0, 1, 2 the copies of A1 as hgibbs_load_bed reads them,
 *                                                                     c = 3 a missing call
 * the per-marker counterpart of hgibbs_row_sums: any sum_i f(g_ij) u_ik is a combination of the four.  Scale and quantisation are
 * those of hgibbs_marker_dots (E_k = 52 - e_k with max_i |u_ik| < 2^e_k, E_k = 0 for an all-zero vector, q = llrint(u 2^E_k)); each
 * of the four is the exact integer sum of its q's, rounded to f64 once (times 2^-E_k), class 0 as sum_i q_ik - S1 - S2 - S3 in
 * integers.  The only error is the rounding of u, |S_jkc - sum u| <= n_c max|u_k| 2^-52 over the n_c rows of the class before that
 * one rounding, so a 0/1 vector returns exact counts, S1 + 2 S2 and S0 + S1 + S2 of an integer-valued vector are hgibbs_marker_dots'
 * raw P and Q, and the results are bit-identical for any m0 / count chunking, any value of the option mdots_split and any repeat.
 * The sums use neither mave nor mstd: a monomorphic marker has them like any other.  Needs the marker stats (computed here when
 * they are not).  Refused: K <= 0 or K > 32, a non-finite entry of U, m0 + count > M, a handle without genotypes, several ranks,
 * n_local >= 2^29, buffers that do not fit in free device memory. */
int hgibbs_marker_class_sums(hgibbs_t h, uint32_t m0, uint32_t count, int K, const double* U, double* out /* count x K x 4 */);
int hgibbs_last_marker_class_sums_ms(hgibbs_t h, double* ms);   /* every kernel of the last call, not the host copies */

/* ---- row-weighted Gram matrices of marker sets */
/* Sets in hgibbs_region_var's convention: set s lists the m_s = off[s + 1] - off[s] markers idx[off[s]] .. idx[off[s + 1] - 1] of the
 * loaded BED, in any order, not necessarily contiguous; a marker may belong to several sets.  w: one non-negative weight per
 * individual of this rank (n_local).  With base_s = sum_{s' < s} m_s'^2, q_i = llrint(w_i 2^E) (hgibbs_marker_dots' scale rule, one
 * E for the vector: E = 52 - e with max_i w_i < 2^e, 0 for an all-zero w), g in {0, 1, 2} the stored genotype and c in {0, 1}
 * "called", for positions a, b of set s:
 *   raw[(base_s + a m_s + b)*3 + 0] = GG_ab = 2^-E sum_i q_i g_ia g_ib      (a missing call contributes 0)
 *   raw[(base_s + a m_s + b)*3 + 1] = GC_ab = 2^-E sum_i q_i g_ia c_ib
 *   raw[(base_s + a m_s + b)*3 + 2] = CC_ab = 2^-E sum_i q_i c_ia c_ib
 *   out[base_s + a m_s + b] = (sd_a sd_b) (((GG_ab - m_b GC_ab) - m_a GC_ba) + (m_a m_b) CC_ab)
 * with m = mave and sd = mstd of the markers, every operation in f64 in this order; out is NaN where either mstd is not finite.  It
 * is sum_i w_i x_ia x_ib for the chain's standardised x (0 at a missing call).  raw may be NULL.  Every raw sum is an exact integer,
 * rounded to f64 once; the only error before the combination is the rounding of w:
 * |GG - sum w g_a g_b| <= 2 n 2^-E <= 4 n max(w) 2^-52, |GC - ..| <= n 2^-E, |CC - ..| <= n 2^-E / 2, each before its one rounding.
 * So the results are bit-identical for any repeat, any batching of the sets over calls, any order of the sets and any value of the
 * option sgram_split (ranges of individuals split over workgroups, 0 = automatic).  Needs the marker stats (computed here when they
 * are not).  Refused, by name: nsets = 0, an empty set, a set of more than 1024 markers, an index >= M, an index listed twice within
 * one set, a non-finite or negative entry of w, a handle without genotypes, several ranks, n_local >= 2^29, buffers that do not fit
 * in free device memory. */
int hgibbs_set_gram(hgibbs_t h, uint32_t nsets, const uint64_t* off /* nsets + 1 */, const uint32_t* idx /* off[nsets] marker indices */,
                    const double* w /* n_local */, double* out, double* raw /* may be NULL */);
int hgibbs_last_set_gram_ms(hgibbs_t h, double* ms);   /* every kernel of the last call, not the host copies; 0 after a refused call */

/* Burden and SKAT statistics of one marker set (host only: no handle, no device; hg_settest.cpp).  U: the m scores; Phi: their
 * m x m covariance under the null model (symmetric, the upper triangle is read); a: the m weights.
 *   burden  t_burden = (sum a_j U_j)^2 / (a'Phi a), p_burden = erfc(sqrt(t_burden / 2)); both NaN when
 *           a'Phi a <= 1e-9 sum a_j^2 Phi_jj.
 *   SKAT    q = sum a_j^2 U_j^2; lam: the eigenvalues of diag(a) Phi diag(a) by cyclic Jacobi, those above 1e-10 lam_max kept, neig
 *           their number, lam_sum and lam_max their sum and largest.  With neig = 0 these fields are NaN and skat_ok = 0.
 *           p_skat = P(sum_k lam_k chi^2_1 >= q) by the saddlepoint approximation in hgibbs_spa_pvalue's Barndorff-Nielsen form:
 *           K(z) = -1/2 sum log(1 - 2 z lam_k), the root of K'(z) = q on (-inf, 1 / (2 lam_max)) by hgibbs_spa_roots' bracketed
 *           Newton rule and stop rule (every sum over the sorted eigenvalues in order: bit-reproducible),
 *           w = sign(z) sqrt(2 (z q - K)), v = z sqrt(K''), p = erfc((w + log(v / w) / w) / sqrt 2) / 2; for
 *           |q - lam_sum| < 1e-6 sqrt(2 sum lam^2) the form's limit erfc(rho / (6 sqrt 2)) / 2, rho = K'''(0) / K''(0)^(3/2) (to first
 *           order 1/2 - rho / (6 sqrt(2 pi))).
 *           skat_ok = 1 when the tail is valid by hgibbs_spa_pvalue's rules, the sign rule excepted: the argument keeps its sign here,
 *           and between the median and the mean of the sum it is positive while z is negative (or the limit was taken); otherwise skat_ok = 0 and
 *           p_skat is the normal tail of (q - lam_sum) / sqrt(2 sum lam^2).
 * Refused: a null argument, m = 0, a non-finite entry of U, a or the upper triangle of Phi. */
typedef struct { double q, p_skat, t_burden, p_burden, lam_sum, lam_max; int32_t neig, skat_ok; } hgibbs_set_result;
int hgibbs_set_tests(uint32_t m, const double* U /* m */, const double* Phi /* m x m, symmetric */, const double* a /* m weights */, hgibbs_set_result* r);

/* The null model of a logistic score test (host only: no handle, no device; hg_logit.cpp).  Z: n x q column-major, first column all
 * ones; y: n entries in {0, 1}.  Newton / IRLS in f64 from coefficients 0, every sum in row order (bit-reproducible), the step halved
 * while the deviance rises (by more than 1e-12 of itself: less is the rounding of its sum).  Stop rule: when max_a |score_a| / sqrt(info_aa) <= 1e-10 one more full step is taken and the fit ends;
 * at most 50 steps.  coef: the q coefficients; mu: the n fitted probabilities; w = mu (1 - mu); chol: q x q column-major, the lower
 * Cholesky factor of Z'WZ at coef (zero above the diagonal); iters: the steps taken (may be NULL).  Refused, each by name: a null
 * argument, q outside 1..64, a non-finite Z, a first column that is not all ones, fewer rows than q + 2, a y outside {0, 1},
 * "dependent columns" (Z'WZ without a Cholesky factor: a pivot at or below 1e-10 of its diagonal entry), "separation" (no
 * convergence within 50 steps, or every row fitted to within 1e-6 of its y). */
int hgibbs_logit_null(uint32_t n, int q, const double* Z, const double* y, double* coef, double* mu, double* w, double* chol, int* iters);

/* ---- saddlepoints of the logistic score test, per listed marker */
/* One record per entry of a marker list.  [0] is the tail at tau = +|s|, [1] the tail at tau = -|s|. */
typedef struct {
    double t[2], K[2], K2[2];   /* [0] the tail at +|s|, [1] at -|s|: saddlepoint, K and K'' there */
    double k2_0, s_lo, s_hi;    /* K''(0) and the open range of K': a tau outside it has no saddlepoint */
    int32_t iters[2];           /* passes after pass 0 */
    uint32_t flags;             /* bit 0/1: tail converged; bit 2/3: tail unreachable */
    uint32_t reserved_;
} hgibbs_spa_root;

/* For entry e of the list: marker j = markers[e] of the loaded BED (any index below M, in any order, duplicates allowed: the entries
 * are independent), the null model's rows Z (n_local x q column-major, Z[k*n_local + i], as hgibbs_logit_null takes it) and mu (fitted
 * probabilities strictly inside (0, 1)), and the entry's own B[e*q + k] = b_k, xv[e*4 + c] (the value of genotype code c; code 3 is a
 * missing call) and score s[e].  With a_i = xv[code_ij] - sum_k Z_ik b_k and u = a_i t, under d_i ~ Bernoulli(mu_i),
 *   K(t) = sum_i [log(1 - mu_i + mu_i e^u) - u mu_i],  K'(t) = sum_i a_i (p_i - mu_i),  K''(t) = sum_i a_i^2 p_i (1 - p_i),
 *   p_i = mu_i e^u / (1 - mu_i + mu_i e^u),
 * each term in the branch-free stable form on E = expm1(-|u|).  Pass 0 gives k2_0 = K''(0), c = sum a_i mu_i,
 * s_hi = sum max(a_i, 0) - c and s_lo = sum min(a_i, 0) - c; a tail whose tau is not strictly inside (s_lo, s_hi) is flagged
 * unreachable and not iterated.  Root rule per tail, both tails in the same passes over the rows: start at t = tau / k2_0 with the
 * open bracket (0, inf) resp. (-inf, 0); the sign of K'(t) - tau tightens the bracket; the proposal is t' = t - (K' - tau) / K''; first
 * the stop rule |t' - t| <= 1e-9 max(|t|, 1 / sqrt(k2_0)) (the tail takes t', one more pass gives K(t') and K''(t'), the converged flag
 * is set), only then the safeguard (a t' not strictly inside the bracket becomes its midpoint when both ends are finite, else 2 t).
 * At most 64 passes per entry after pass 0; a tail still open then has neither flag.  Every sum over the rows runs in one fixed
 * order that depends on n_local only (a fixed stride per thread, a fixed tree in the workgroup, no atomics): the records are
 * bit-identical for any chunking of the list, any position of an entry in it and any repeat.  Padding slots past n_local take no
 * part.  nm = 0 returns 0 and touches nothing.  Refused: a null argument, q outside 1..64, a marker index >= M, a non-finite entry of
 * Z, B, xv or s, a mu not strictly inside (0, 1), several ranks, a handle without genotypes, buffers that do not fit in free device
 * memory. */
int hgibbs_spa_roots(hgibbs_t h, uint32_t nm, const uint32_t* markers, int q, const double* Z /* n_local x q column-major, as hgibbs_logit_null */,
                     const double* mu, const double* B /* nm x q */, const double* xv /* nm x 4 */, const double* s /* nm */, hgibbs_spa_root* out);
int hgibbs_last_spa_ms(hgibbs_t h, double* ms);   /* every kernel of the last call, not the host copies; 0 after a refused call */

/* The saddlepoint p-value from a record of hgibbs_spa_roots (host only: no handle, no device; hg_spa.cpp), Barndorff-Nielsen form.
 * Per tail, with tau = +|s| resp. -|s|, t, K = K(t), K2 = K''(t):  w = sign(t) sqrt(2 (t tau - K)),  v = t sqrt(K2),
 * z = w + log(v / w) / w,  tail = erfc(|z| / sqrt 2) / 2.  A tail is valid only if it converged, t tau - K > 0, K2 > 0, v / w > 0 and
 * z is finite with tau's sign; a tail that underflows to 0 is valid.  p_upper, p_lower (either may be NULL): the tails, NaN where not
 * valid; p = p_upper + p_lower and valid = 1 when both are valid, else p = NaN and valid = 0 (valid may be NULL): the caller keeps
 * the normal approximation then.  Refused: a null r or p. */
int hgibbs_spa_pvalue(double s, const hgibbs_spa_root* r, double* p_upper, double* p_lower, double* p, int* valid);

/* ---- Firth's penalised fit of the logistic score test's one-parameter model, per listed marker */
/* One record per entry of a marker list. */
typedef struct {
    double beta;       /* the stationary point of l* the rule found, in units of a */
    double K, K2;      /* K(beta), K''(beta) from the closing pass (0 unless converged) */
    double g;          /* the modified score at the last iterated point */
    double k2_0;       /* K''(0) = the score test's V */
    int32_t iters;     /* passes after pass 0, the closing one included */
    uint32_t flags;    /* bit 0 converged; bit 1 degenerate (k2_0 not finite or <= 0: not iterated, every other field 0) */
} hgibbs_firth_rec;

/* The inputs are those of hgibbs_spa_roots, entry by entry (markers, Z, mu, B, xv; a_i, u = a_i t, p_i and the stable form of the terms
 * as there), and s[e] is the entry's score sum_i a_i (d_i - mu_i): the operator never sees d.  In the model
 * logit P(d_i = 1) = logit(mu_i) + beta a_i the log-likelihood ratio is l(t) - l(0) = t s - K(t), and Firth's penalised one is
 * l*(t) - l*(0) = t s - K(t) + log(K''(t) / K''(0)) / 2.  With v = p (1 - p),
 *   K''' = sum_i a_i^3 v_i (1 - 2 p_i),  K'''' = sum_i a_i^4 v_i (1 - 6 v_i),
 *   g(t) = s - K' + K''' / (2 K''),  g'(t) = -K'' + (K'''' / K'' - (K''' / K'')^2) / 2.
 * Root rule, Newton on g with a bracket: pass 0 is at t = 0 and gives k2_0 and scale = 1 / sqrt(k2_0) (a k2_0 that is not finite or not
 * positive sets the degenerate flag and ends the entry); lo = -inf, hi = +inf, tg = 0.  When g and g' are finite at t: tg = t, g > 0
 * sets lo = t, g < 0 sets hi = t, the proposal is t' = t - g / g'; first the stop rule g' < 0 and |t' - t| <= 1e-9 max(|t|, scale) (the entry takes
 * t', one closing pass gives K(t') and K''(t'), the converged flag is set), only then the safeguard (a t' not strictly inside (lo, hi)
 * becomes the midpoint when both ends are finite, else 2 t, or +-scale with g's sign when t = 0).  When g or g' is not finite at t (the
 * probabilities have saturated): the bracket end on t's side of tg becomes t, the next point is (t + tg) / 2, no sign is taken.  At
 * most 64 passes after pass 0, the closing one included; an entry still open then has no flag, and beta is the point the rule would
 * have taken next.  l* can have more than one stationary point: the record is the one this rule reaches from 0.  Any finite s is
 * taken; for an s outside the range of K' (section 26's [s_lo, s_hi]), which no phenotype gives, l* need not have a maximum and only
 * the bound on the passes is promised.
 * Every sum over the rows runs in hgibbs_spa_roots' order, which depends on n_local only.  Pass 0 writes a_i to a scratch row per
 * entry (n_local doubles) that the later passes read; the list is processed in pieces of entries so that the scratch fits: option
 * firth_piece.  The records are bit-identical for any firth_piece, any chunking of the list, any position of an entry in it, duplicates
 * and repeats.  nm = 0 returns 0 and touches nothing.  Refused: a null argument, q outside 1..64, a marker index >= M, a non-finite
 * entry of Z, B, xv or s, a mu not strictly inside (0, 1), several ranks, a handle without genotypes, buffers that do not fit in free
 * device memory. */
int hgibbs_firth_fit(hgibbs_t h, uint32_t nm, const uint32_t* markers, int q, const double* Z /* n_local x q column-major, as hgibbs_logit_null */,
                     const double* mu, const double* B /* nm x q */, const double* xv /* nm x 4 */, const double* s /* nm */, hgibbs_firth_rec* out);
int hgibbs_last_firth_ms(hgibbs_t h, double* ms);   /* every kernel of the last call, not the host copies; 0 after a refused call */

/* The statistics of a record of hgibbs_firth_fit (host only: no handle, no device; hg_firth.cpp).
 * lrt = 2 (beta s - K + log(K2 / k2_0) / 2), a value in [-1e-9, 0) becomes 0;  se = 1 / sqrt(K2);  p = erfc(sqrt(lrt / 2)).
 * valid = 1 iff the record is converged and not degenerate, K2 > 0 and lrt is finite and >= 0 after the clamp; otherwise valid = 0 and
 * lrt, se and p are NaN: the caller keeps the score test.  lrt, se and valid may be NULL.  Refused: a null r or p. */
int hgibbs_firth_stats(double s, const hgibbs_firth_rec* r, double* lrt, double* se, double* p, int* valid);

/* ---- KING-robust kinship of the loaded rows -------- */
/* For rows a, b of the handle (the n_local rows kept at hgibbs_load_bed), over the markers where both calls are present, five exact
 * counts in this order: NSNP (called in both), HET_a, HET_b (a, resp. b, heterozygous among those), HETHET (both heterozygous), IBS0
 * (one homozygous 0, the other homozygous 2); KINSHIP = 1/2 - (4 IBS0 + (HET_a - HETHET) + (HET_b - HETHET)) / (4 min(HET_a, HET_b)),
 * NaN when min(HET_a, HET_b) = 0.  One rank only; M < 2^31.  The counts are exact integers: bit-identical for any blocking and any
 * value of the option king_split (ranges of markers split over workgroups, 0 = automatic).  The call builds an individual-major copy
 * of the codes on the device (the size of the loaded BED) and refuses, with a message, when it does not fit in free memory.
 *
 * hgibbs_king: counts[((a - a0) * bcount + (b - b0)) * 5 + t] for a in [a0, a0 + acount), b in [b0, b0 + bcount); any offsets, a == b
 *   allowed (HET_a = HET_b = HETHET there). */
int hgibbs_king(hgibbs_t h, uint32_t a0, uint32_t acount, uint32_t b0, uint32_t bcount, int32_t* counts);
/* hgibbs_king_pairs: every pair a < b with KINSHIP >= cutoff (finite; NaN pairs never pass); *npairs = their number.  The list is
 *   grown inside the call when it overflows (no pair is dropped) and kept in the handle, sorted by (a, b), until the next call. */
int hgibbs_king_pairs(hgibbs_t h, double cutoff, uint64_t* npairs);
/* copies the list out: ab[2 p], ab[2 p + 1] = a, b; counts[5 p + t]; kin[p].  Any pointer may be NULL. */
int hgibbs_king_pairs_get(hgibbs_t h, uint32_t* ab, int32_t* counts, double* kin);
/* device time of the last hgibbs_king / hgibbs_king_pairs in ms: every kernel of the call (image, zeroing, products, every run of the
 * list), not the host copies or the allocations */
int hgibbs_last_king_ms(hgibbs_t h, double* ms);

/* ---- runs of homozygosity of the loaded rows ------- */
/* PLINK 1.9's --homozyg scan restated in integers, for every row of the handle over a list of runs: run r is the entries
 * [run_off[r], run_off[r + 1]) of idx (markers of the handle, ascending) and bp (not decreasing), run_off[0] = 0; a position is an entry.
 * Codes: 1 = het, 3 = missing call.  Within a run of L entries window s covers the positions [s, s + window), 0 <= s <= L - window, and
 * is homozygous when it holds at most window_het hets and at most window_missing missing calls.  A position that lies in n windows is
 * covered when at least need[n] of them are homozygous (the caller's table: the smallest c with (double)c / (double)n >= threshold;
 * need[0] is not read).  A segment is a maximal stretch of covered positions, also cut between neighbours whose bp differ by more than
 * gap_bp.  Segment [first, last] with nsnp = last - first + 1 and len = bp[last] - bp[first] is kept iff nsnp >= min_snps, len >= min_bp,
 * len <= dens_bp nsnp (in 64 bits) and, unless max_het is UINT32_MAX, nhet <= max_het.  A run shorter than the window has no segment.
 * Integers only: the list is bit-identical for any capacity of the list and any repeat.  One rank only.  Refused: a handle without
 * genotypes, several ranks, a null argument, window outside 1..64, need[n] outside 1..n for an n in 1..window, a marker index >= M, idx
 * not ascending or bp decreasing within a run, bp outside 0..2^62, a negative limit, more than 65535 runs, 2^31 entries or more,
 * buffers that do not fit in free device memory.  A refused call leaves the previous list alone. */
typedef struct { uint32_t window, window_het, window_missing; uint32_t need[65]; uint32_t min_snps;
                 int64_t min_bp, dens_bp, gap_bp; uint32_t max_het /* UINT32_MAX: none */; } hgibbs_roh_params;
typedef struct { uint32_t row, first, last /* positions in idx, inclusive */, nsnp, nhet, nmiss; } hgibbs_roh_seg;
/* *nseg = the number of kept segments.  The list is an atomic append, counted in full: when it overflows its first capacity (option
 * roh_list0) the kernel runs once more with the exact one; it is kept in the handle, sorted by (row, first), until the next call. */
int hgibbs_roh(hgibbs_t h, uint32_t nruns, const uint32_t* run_off /* nruns + 1 */, const uint32_t* idx /* run_off[nruns] markers, ascending within a run */,
               const int64_t* bp /* per entry of idx */, const hgibbs_roh_params* p, uint64_t* nseg);
int hgibbs_roh_get(hgibbs_t h, hgibbs_roh_seg* segs);   /* sorted by (row, first); kept on the handle until the next call */
int hgibbs_last_roh_ms(hgibbs_t h, double* ms);         /* every kernel of the last call, not the host copies; 0 after a refused call */

/* ---- joint genotype tables of pairs of markers, and the epistasis screen ------- */
/* hgibbs_pair_tables: for every a < na and b < nb, tables[((a * nb + b) * 2 + k) * 9 + 3 * i + j] = the number of the handle's rows of
 * class k at which marker idxA[a] has stored code i and marker idxB[b] has stored code j, i and j in {0, 1, 2} as hgibbs_load_bed reads
 * them.  A row with a missing call at either marker is counted in no cell; padding slots count nowhere.  cls gives the class (0 or 1)
 * of each of the n_local rows; NULL puts every row into class 0 (the class-1 tables are then zero).  The lists are arbitrary: unordered,
 * with holes, the same marker on both sides (the table is then diagonal) or twice in a list.  Every cell is an exact integer: the result
 * is bit-identical for any tiling, any value of the option ptab_split, any cut of the lists over calls and any repeat.  One rank only.
 * Refused: a null handle, list or result; na or nb equal to 0; an index >= M; an entry of cls above 1; a handle without genotypes;
 * several ranks; n_local >= 2^29; buffers (72 bytes a pair) that do not fit in free device memory.  Computes the marker stats when the
 * handle has none yet. */
int hgibbs_pair_tables(hgibbs_t h, uint32_t na, const uint32_t* idxA, uint32_t nb, const uint32_t* idxB,
                       const uint8_t* cls /* n_local: 0 or 1; NULL = every row class 0 */, int32_t* tables /* na x nb x 18 */);
int hgibbs_last_pair_tables_ms(hgibbs_t h, double* ms); /* every kernel of the last call, not the host copies; 0 after a refused call */
/* hgibbs_epi_scan: BOOST's screen over the pairs (a, b) of list positions -- with idxB every a < na against every b < nb, with idxB NULL
 * the pairs a < b of list A -- in blocks of the pair space: a block's tables are made as above, a second kernel evaluates the Kirkwood
 * superposition bound KSA of each pair from its 18 counts in f64 (the operations of hgibbs_epi_test's ksa, in the same order), and the
 * pair is appended to a list when KSA >= threshold - delta, delta = 2^-44 * 2 n (4 ln n + ln 18) with n = n_local: the bound of the
 * evaluation's rounding, so that no pair whose exact KSA reaches the threshold is lost.  Only the list crosses the bus.  The list is an
 * atomic append counted in full: when it overflows its first capacity (option epi_list0) the scan runs once more with the exact one.  It
 * is kept in the handle, sorted by (a, b), until the next call; *npairs = its length.  A pair's value depends on its integer table
 * alone: the list is identical for any ptab_split, any block size (option epi_block) and any repeat.  The host synchronises with the
 * device after each block's products and after its screen, an overflow of the list recomputes every block, and a scan with idxB NULL
 * computes its diagonal blocks in full: harmless at the default block size, and the reason epi_block is a test knob.  Refused: threshold not finite or
 * <= 0, a null npairs, and everything hgibbs_pair_tables refuses.  A refused call leaves the previous list alone. */
int hgibbs_epi_scan(hgibbs_t h, uint32_t na, const uint32_t* idxA, uint32_t nb, const uint32_t* idxB /* NULL: pairs a < b of list A */,
                    const uint8_t* cls, double threshold, uint64_t* npairs);
/* copies the list out: ab[2 p], ab[2 p + 1] = the positions a, b in the lists; tables[18 p + 9 k + 3 i + j]; ksa[p] the device's
 * value.  Any pointer may be NULL. */
int hgibbs_epi_scan_get(hgibbs_t h, uint32_t* ab /* 2 per pair: positions in the lists */, int32_t* tables /* 18 per pair */, double* ksa);
/* device time of the last hgibbs_epi_scan in ms, every run of the list: the products (class image, marker counts, tables) and the
 * screen; both 0 after a refused call.  Either pointer may be NULL. */
int hgibbs_last_epi_ms(hgibbs_t h, double* products_ms, double* screen_ms);
/* hgibbs_epi_test (hg_epi.cpp: no device, no handle): BOOST's interaction test of one table18[9 k + 3 i + j].  ksa: the Kirkwood bound
 * 2 (sum n log(n_ijk / n) - sum n log p^K_ijk), p^K = pi_ij. pi_i.k pi_.jk / (pi_i.. pi_.j. pi_..k) / eta, over the cells n_ijk > 0.
 * lr = 2 (L_S - L_H) >= 0: L_H the log-likelihood of the homogeneous-association model fitted by iterative proportional fitting from a
 * table of ones, cycling over the ij, ik, jk margins, until no cell moves by more than 1e-10 n in a cycle (converged = 1) or 2000 cycles
 * are done (converged = 0: lr is then an upper bound); iters = the cycles.  df = (I - 1)(J - 1) with I, J the codes of each marker that
 * occur: 0, 1, 2 or 4; df = 0 gives lr = 0, iters = 0, converged = 1, p = NaN.  p: erfc(sqrt(lr / 2)), exp(-lr / 2),
 * exp(-lr / 2) (1 + lr / 2) for df = 1, 2, 4.  Refused: a null argument, a negative count. */
typedef struct { double ksa, lr; int df, iters, converged; double p; } hgibbs_epi_result;
int hgibbs_epi_test(const int32_t* table18, hgibbs_epi_result* r);

/* ---- principal components of the loaded rows ------- */
/* The top K eigenpairs of A = X X' / M_used over the handle's n_local rows, X the chain's standardised genotypes (hgibbs_marker_stats;
 * x = 0 at a missing call; a marker without a finite mstd contributes nothing and is not counted in M_used), by block subspace
 * iteration on a panel of L vectors (K <= L <= 32) with a final Rayleigh-Ritz step.  A is never formed: an iteration is T = X'Q through
 * the kernels of hgibbs_marker_dots and Y = X T through those of hgibbs_score, on panels that stay in device memory; Y is made
 * orthonormal by CholeskyQR done twice.  The call stops after `iters` iterations or, for tol > 0, when the largest relative change of
 * the first K Ritz values between two iterations is <= tol.
 *   Q0        L x n_local start vectors (vector-major), or NULL: then entry (k, i) comes from a counter hash of (seed, k, i)
 *   eigval    K eigenvalues of A, descending
 *   pcs       K x n_local, unit length, orthonormal; the entry of largest magnitude of each is positive (lowest index on a tie)
 *   loadings  K x M unit-length right singular vectors X'v_k / sqrt(M_used lambda_k), NaN outside M_used; or NULL
 *   rep       iterations run, M_used, the last relative change of the Ritz values (HUGE_VAL after one iteration) and
 *             resid[k] = |A v_k - lambda_k v_k| / lambda_k from one more pair of products; or NULL (no residuals, no products)
 * The products are exact integer operators and every floating-point sum of the panel algebra runs in a fixed order: for given
 * arguments the results are bit-identical whatever the options mdots_split, score_sp and score_ranges say.  Refused with a message:
 * several ranks, no genotypes, K < 1, K > L, L > 32, L >= n_local, L > M_used, iters < 1, tol negative or not finite, a non-finite
 * Q0, n_local >= 2^29, panels that do not fit in free device memory, a panel that loses rank. */
typedef struct {
    int32_t iters_run;
    uint32_t m_used;
    double ritz_change;
    double resid[32];
} hgibbs_pca_report;
int hgibbs_pca(hgibbs_t h, int K, int L, int iters, double tol, const double* Q0, uint64_t seed, double* eigval, double* pcs,
               double* loadings, hgibbs_pca_report* rep);
/* device time of the last hgibbs_pca in ms, kernels only: ms4[0] the whole call, [1] the X'Q products, [2] the X T products, [3] the
 * panel algebra of the iterations (fold, Gram matrices, CholeskyQR); the start panel, the final step and the residuals are in [0] only */
int hgibbs_last_pca_ms(hgibbs_t h, double* ms4);

/* ---- genomic relationship matrix of the loaded rows -- */
/* S = X X' over the handle's n_local rows, X the chain's standardised genotypes (x = 0 at a missing call), and the number of markers
 * both rows are called at: the GCTA entry is A_ab = S_ab / NSNP_ab (NaN when NSNP_ab = 0).  mave_j and mstd_j are those of
 * hgibbs_marker_stats (computed here when they are not), g in {0, 1, 2} the genotype as hgibbs_load_bed reads it.
 *   A marker is USED when mstd_j is finite; M_used is their number.  Per used marker and genotype g, two f64 values, every operation
 *   rounded to f64 on its own (no fused multiply-add):   y_jg = (mstd_j * mstd_j) * (g - mave_j),   z_jg = mave_j * y_jg.
 *   W = the largest |y| or |z| of that table, e the smallest integer with W < 2^e, E = 52 - e (0 for an all-zero table);
 *   qy = llrint(y 2^E), qz = llrint(z 2^E).  For a >= b (row a is the weight side, b the code side):
 *     T_ab    = sum over used j with a and b called of ( g_bj qy[j][g_aj] - qz[j][g_aj] )      an exact integer
 *     S_ab    = T_ab 2^-E, rounded to f64 once
 *     NSNP_ab = the number of used j with a and b called
 *   |S_ab - exact| <= 1.5 M_used 2^-E <= 3 M_used W 2^-52.
 * hgibbs_grm covers rows a in [a0, a0 + acount), each with its columns b = 0 .. a, packed in GCTA's order: row a0 first, then row
 * a0 + 1, ...: sum of (a + 1) entries.  Either output pointer may be NULL.  Every sum is an integer: the results are bit-identical for
 * any chunking of the rows, any value of the option grm_split (ranges of markers split over workgroups, 0 = automatic; the parts meet
 * in i32 atomic adds of the per-digit accumulators) and any repeat.  A call of more than 2^25 pairs works in pieces of rows (option
 * grm_piece: another number of pairs per piece, 0 = 2^25; a row alone may exceed it; the results do not depend on it).  The
 * call builds an individual-major copy of the codes on the device (the size of the loaded BED).  Refused with a message: several
 * ranks, no genotypes, acount = 0, a0 + acount > n_local, M_used = 0, M > 5 592 405 (a per-digit sum is at most 384 M and stays
 * inside an i32), more rows than hgibbs_king takes, buffers that do not fit in free device memory. */
int hgibbs_grm(hgibbs_t h, uint32_t a0, uint32_t acount, double* S, int32_t* nsnp);
/* M_used and E of the last hgibbs_grm or hgibbs_grm_rowsums (0, 0 after a refused call of either); either pointer may be NULL */
int hgibbs_grm_info(hgibbs_t h, uint32_t* m_used, int32_t* E);
/* device time of the last hgibbs_grm in ms: every kernel of the call (scale, table, image, zeroing, products, rounding), not the host
 * copies or the allocations */
int hgibbs_last_grm_ms(hgibbs_t h, double* ms);

/* ---- row sums of the relationship matrix and Haseman-Elston regression -- */
/* What a regression on the off-diagonal entries needs of the matrix, reduced on the device: the triangle never reaches the host.
 * S_ab and NSNP_ab are exactly hgibbs_grm's over all n_local rows.  For a != b with NSNP_ab > 0, A_ab = S_ab / (double)NSNP_ab (one IEEE
 * division); such b are the PARTNERS of a.  k is the smallest integer with n_local <= 2^k, F = 58 - k, fx(t) = llrint(t 2^F).  Per row a,
 * the sums running over its partners b:
 *     AY[a][p]    = sum fx(A_ab * Y[p][b])      (one f64 product, then the exact scaling)
 *     A1[a]       = sum fx(A_ab)
 *     A2[a]       = sum fx(A_ab * A_ab)
 *     partners[a] = their number
 *     diag[a]     = S_aa / NSNP_aa, NaN when NSNP_aa = 0
 * Y: P vectors over the rows, vector-major (Y[p*n_local + b]), 1 <= P <= 8, every entry finite.  ay[a*P + p], a1[a], a2[a] are
 * (double)sum 2^-F, converted once; any output pointer may be NULL.  |ay - sum A_ab Y_pb| <= partners 2^-(F+1) beyond the rounding of each
 * product and the one conversion.
 *   Range: every term t (A_ab Y[p][b], A_ab, A_ab^2) must satisfy |t| < 16; then |fx(t)| <= 2^(62 - k) and a row's sum of fewer than 2^k
 *   terms stays below 2^62.  The device keeps the largest |t| it met; when that is >= 16 the call is refused after the run, the message
 *   names the magnitude, and no output is touched.  Nothing wraps silently.
 * Every sum is an integer sum of per-pair integers: the results are bit-identical for any value of the options grm_split and grm_piece,
 * any tile shape, any launch order and any repeat, and column p of a call with P vectors equals the call with P = 1 and that vector.
 * The products are hgibbs_grm's kernels on pieces of rows of at most grm_piece pairs; a reducer sums each piece where it lies, into an
 * n_local x (P + 3) accumulator of signed 64-bit integers.  Refused with a message: several ranks, no genotypes, n_local < 2, P outside
 * 1..8, a null or non-finite Y, M > 5 592 405, M_used = 0, more rows than hgibbs_king takes, buffers that do not fit in free device
 * memory, the range rule.  The handle serves every other operator after any refusal. */
int hgibbs_grm_rowsums(hgibbs_t h, int P, const double* Y, double* ay, double* a1, double* a2, double* diag, uint32_t* partners);
/* device time of the last hgibbs_grm_rowsums in ms: the products (every kernel hgibbs_grm would run: scale, table, image, zeroing,
 * products, rounding) and the reduce (zeroing the accumulator, the reduction kernel of every piece, the final conversion); not the
 * host copies.  0, 0 after a refused call, whether it was refused before the device work or after it (the range rule) */
int hgibbs_last_grm_rowsums_ms(hgibbs_t h, double* products_ms, double* reduce_ms);

/* Haseman-Elston regression from those row sums (host only: no handle, no device).  Inputs over n rows: y, ay = A y, ayy = A (y o y),
 * a1, a2, partners, as hgibbs_grm_rowsums gives them for Y = [y, y o y].  Rows with partners = 0 are left out and counted; n' rows
 * remain and each must have partners = n' - 1 (refused otherwise, naming the first row that has not), so that the pairs are all
 * m = n'(n' - 1)/2 pairs of the used rows.  Over those pairs z is regressed on A by OLS with an intercept, for z = y_a y_b (HE-CP) and
 * z = (y_a - y_b)^2 (HE-SD), from closed forms of sum A, sum A^2, sum z, sum A z, sum z^2 in the row sums and the power sums of y:
 *   slope = (m sum Az - sum A sum z) / D, D = m sum A^2 - (sum A)^2;  intercept = (sum z - slope sum A) / m;
 *   s^2 = (sum z^2 - intercept sum z - slope sum Az) / (m - 2);  SE^2(slope) = s^2 m / D;  SE^2(intercept) = s^2 sum A^2 / D.
 * The jackknife deletes one individual at a time (its n' - 1 pairs leave every sum, in closed form): SE_jk^2 = (n' - 1)/n' sum (theta_(-a)
 * - mean)^2.  Vp = sum (y - ybar)^2 / (n' - 1) over the used rows; h2 = slope / Vp for CP and -slope / (2 Vp) for SD, and the SEs of h2
 * are the slope's scaled the same way: Vp IS TAKEN AS FIXED.  The P values are two-sided normal (erfc) of estimate / SE; h2's are the
 * slope's.  Refused with a message: a null argument, n' < 4, a non-finite input in a used row, a constant y, D <= 0. */
typedef struct {
    double intercept, slope, h2;
    double intercept_se, slope_se, h2_se;          /* OLS */
    double intercept_se_jk, slope_se_jk, h2_se_jk; /* delete-one-individual jackknife */
    double intercept_p, slope_p;                   /* from the OLS SEs */
    double intercept_p_jk, slope_p_jk;             /* from the jackknife SEs */
} hgibbs_he_form;
typedef struct {
    uint32_t n_used;     /* n' */
    uint32_t n_left_out; /* rows with partners = 0 */
    uint64_t pairs;      /* m */
    double vp;
    hgibbs_he_form cp, sd;
} hgibbs_he_result;
int hgibbs_he_fit(uint32_t n, const double* y, const double* ay, const double* ayy, const double* a1, const double* a2,
                  const uint32_t* partners, hgibbs_he_result* out);

/* ======================================================================== */
/* Host driver: the body of BayesRRm::runMpiGibbs (src/BayesRRm.cpp:933-2939)
 * for --mpibayes bayesMPI, restated on top of hgibbs_*.                     */
/* ======================================================================== */
typedef struct hydra_chain* hydra_chain_t;

typedef struct {
    uint32_t seed;          /* --seed */
    int32_t shuffle;        /* --shuf-mark */
    int32_t G, K;           /* groups, mixture components incl. the zero one */
    const int32_t* groups;  /* M, or NULL for one group (src/BayesRRm.cpp:984-996) */
    const double* mS;       /* G*K, column 0 == 0.0 */
} hydra_model_desc;

/* y_host: phenotypes of the kept individuals of ALL ranks (n_global entries,
 * NA rows removed); the chain centres/scales it (src/BayesRRm.cpp:1564-1579). */
int hydra_chain_create(hgibbs_t dev, const hydra_model_desc* model, const double* y_host, hydra_chain_t* out);
int hydra_chain_destroy(hydra_chain_t c);
/* optional fixed effects (--covariates): X_host = n_global x C row-major, same
 * individuals and order as y_host; call once before the first iteration */
int hydra_chain_set_covariates(hydra_chain_t c, const double* X_host, int C);
int hydra_chain_gamma(hydra_chain_t c, double* gamma_out /* C */, int32_t* xI_out /* C, may be NULL */);
/* one Gibbs iteration: mu, shuffle, sweep, sigmaG/pi per group, covariates, sigmaE */
int hydra_chain_iterate(hydra_chain_t c);
/* hyper-parameters after the last iteration; any pointer may be NULL */
int hydra_chain_state(hydra_chain_t c, double* sigmaE, double* mu, double* sigmaG /*G*/, double* estPi /*G*K*/,
                      int32_t* m0 /*G*/, int32_t* cass /*G*K*/, hgibbs_rng_state* rng);
/* the .csv line of src/BayesRRm.cpp:2742-2760 for the given iteration number */
int hydra_chain_csv_line(hydra_chain_t c, uint32_t iteration, char* buf, size_t len);
const int32_t* hydra_chain_order(hydra_chain_t c);

/* ---- the same chain from summary statistics -------- */
/* hydra_chain's initial values and hyper-parameter draws around hgibbs_ss_sweep: sigmaG ~ beta(1, 1) per group, sigmaE = y'y / n 0.5
 * with y'y = n - 1, n = n_eff; mu ~ N(0, sigmaE / n); e_sqn = (y'y - sum_j beta_j (b_j + c_j)) + n mu^2.  No covariates.  An iteration
 * whose e_sqn is not positive fails with a message that names the iteration and the value (a truncated band need not be positive
 * definite); nothing is clamped.  `use` (M bytes or NULL): 0 = the marker is never adaptive.
 *   create        on a handle that holds the panel: calls hgibbs_ss_begin (which refuses n_eff, W, ahead and xty by name) and
 *                 hgibbs_set_model; the effects are read with hgibbs_get_beta or hydra_ss_chain_effects
 *   create_host   host only, no device: the same iteration around hgibbs_ss_sweep_host with the caller's band (M x W) */
typedef struct hydra_ss_chain* hydra_ss_chain_t;
int hydra_ss_chain_create(hgibbs_t dev, const hydra_model_desc* model, double n_eff, uint32_t W, const uint32_t* ahead, const double* xty,
                          const uint8_t* use, hydra_ss_chain_t* out);
int hydra_ss_chain_create_host(uint32_t M, const hydra_model_desc* model, double n_eff, uint32_t W, const uint32_t* ahead, const double* band,
                               const double* xty, const uint8_t* use, hydra_ss_chain_t* out);
int hydra_ss_chain_destroy(hydra_ss_chain_t c);
int hydra_ss_chain_iterate(hydra_ss_chain_t c);
int hydra_ss_chain_state(hydra_ss_chain_t c, double* sigmaE, double* mu, double* sigmaG /*G*/, double* estPi /*G*K*/, int32_t* m0 /*G*/,
                         int32_t* cass /*G*K*/, hgibbs_rng_state* rng);
/* effects, components, acum and c (M each; any pointer may be NULL) */
int hydra_ss_chain_effects(hydra_ss_chain_t c, double* beta, int32_t* components, double* acum, double* cvec);
uint64_t hydra_ss_chain_last_nnz(hydra_ss_chain_t c);
const int32_t* hydra_ss_chain_order(hydra_ss_chain_t c);
int hydra_ss_chain_csv_line(hydra_ss_chain_t c, uint32_t iteration, char* buf, size_t len);
/* Independent LD blocks in parallel streams, either engine, before the first iteration only: bounds from
 * hgibbs_ss_partition(S_max); stream s is seeded with the generator's seeding rule from w_s, where w_0 .. w_{S-1} are the next S words
 * of the chain's own generator at this call.  From then on an iteration calls hgibbs_ss_sweep_streams(_host); mu, the shuffle, the
 * hyper-parameters and sigmaE stay on the chain's generator.  hydra_ss_chain_streams reads back S (0: single stream), bounds (S + 1)
 * and the S states (any pointer may be NULL). */
int hydra_ss_chain_set_streams(hydra_ss_chain_t c, uint32_t S_max);
int hydra_ss_chain_streams(hydra_ss_chain_t c, uint32_t* S, uint32_t* bounds, hgibbs_rng_state* rngs);

/* R chains on one band of the device: chain r is, bit for bit, the hydra_ss_chain created on the device with
 * model.seed = seeds[r] (model->seed is not read) and, with S_max > 0, hydra_ss_chain_set_streams(S_max): every .csv line, effect,
 * component, acum and generator.  One iteration is one hgibbs_ss_sweep_replicas and one hgibbs_ss_replica_sums between the chains' own
 * draws; an e_sqn that is not positive stops it with hydra_ss_chain_iterate's message and the chain's number.  R in 1..64, S_max in
 * 0..1024 (0: the single stream).  No host engine: R host chains are R hydra_ss_chain_create_host calls.
 *   streams   S (0: single stream), bounds (S + 1) and the R x S states, chain-major (any pointer may be NULL) */
typedef struct hydra_ss_multi* hydra_ss_multi_t;
int hydra_ss_multi_create(hgibbs_t dev, const hydra_model_desc* model, uint32_t R, const uint32_t* seeds /* R */, double n_eff, uint32_t W,
                          const uint32_t* ahead, const double* xty, const uint8_t* use, uint32_t S_max, hydra_ss_multi_t* out);
int hydra_ss_multi_destroy(hydra_ss_multi_t c);
int hydra_ss_multi_iterate(hydra_ss_multi_t c);
int hydra_ss_multi_state(hydra_ss_multi_t c, uint32_t r, double* sigmaE, double* mu, double* sigmaG /*G*/, double* estPi /*G*K*/, int32_t* m0 /*G*/,
                         int32_t* cass /*G*K*/, hgibbs_rng_state* rng);
int hydra_ss_multi_effects(hydra_ss_multi_t c, uint32_t r, double* beta, int32_t* components, double* acum, double* cvec);
int hydra_ss_multi_streams(hydra_ss_multi_t c, uint32_t* S, uint32_t* bounds, hgibbs_rng_state* rngs);
uint64_t hydra_ss_multi_last_nnz(hydra_ss_multi_t c, uint32_t r);
int hydra_ss_multi_csv_line(hydra_ss_multi_t c, uint32_t r, uint32_t iteration, char* buf, size_t len);

/* ======================================================================== */
/* BayesW: Weibull survival model (src/BayesW.cpp); individuals shard as above  */
/* ======================================================================== */
/* The libc rand() stream the reference's ARS draws from (src/BayesW_arms.cpp:914-919,
 * srand at src/BayesW.cpp:1012, :877, :2029), one private copy per chain:
 * glibc's TYPE_3 additive-feedback generator. */
typedef struct {
    int32_t r[31];
    int32_t f, b;
} hgibbs_grand_state;
void hgibbs_grand_seed(hgibbs_grand_state* st, uint32_t seed); /* srand(seed) */
int32_t hgibbs_grand_next(hgibbs_grand_state* st);             /* rand()      */

/* arms(xinit, 4, &xl, &xr, logdens, data, &convex=1.0, 100, 0, ..., nsamp=1, ...) of
 * src/BayesW_arms.cpp as BayesW calls it: one draw from exp(logdens) on [xl, xr].
 * Returns 0 or the reference's error code (1003, 1004, 2000). */
int hgibbs_ars_sample(const double* xinit4, double xl, double xr, double (*logdens)(double, void*), void* data,
                      hgibbs_grand_state* rng, double* xsamp, int* neval);

typedef struct {
    uint64_t launches;    /* batch launches of the last sweep */
    uint64_t nnz_updates; /* markers whose effect changed */
    uint64_t ars_draws, ars_evals;
    double device_ms;       /* first launch to last, host round trips included */
    double sums_kernel_ms;  /* total of the k_bw_sums launches (option "w_kernel_timing"), else 0 */
} hgibbs_w_sweep_stats;

/* failure indicator (0/1) of the n_global kept individuals; allocates vi next to eps */
int hgibbs_w_init(hgibbs_t h, const int32_t* failure_host);
/* mean, standard deviation (not its inverse) and sum_failure per marker, src/BayesW.cpp:1201-1232 */
int hgibbs_w_marker_stats(hgibbs_t h, double* mave, double* sd, double* sum_failure);
/* groups[M] (NULL = one group), mS: G x K with column 0 == 0 (src/BayesW.cpp:760-790),
 * quad_points in {3,5,7,9,11,13,15,17,25} (:706-708) */
int hgibbs_w_set_model(hgibbs_t h, int G, int K, const int32_t* groups_host, const double* mS, int quad_points);
/* the N-length sums inside the scalar log densities, on the current residual:
 *  kind 0  sum_i exp(((eps_i + p0) - p1) * p2 - EuMasc)                mu_dens,    :77-88
 *  kind 1  sum_i exp(eps_i * p0 - EuMasc)                              alpha_dens, :132-142
 *  kind 2  sum_i exp(((eps_i + x_ic*p0) - x_ic*p1) * p2 - EuMasc)      gamma_dens, :118-129 (c = col)
 *  kind 3  sum_i eps_i * failure_i                                     alpha_dens */
int hgibbs_w_reduce(hgibbs_t h, int kind, int col, double p0, double p1, double p2, double* out);
/* vi_i = exp(alpha * eps_i - EuMasc), src/BayesW.cpp:1457-1459 */
int hgibbs_w_refresh_vi(hgibbs_t h, double alpha);
int hgibbs_w_get_vi(hgibbs_t h, double* vi_host /* n_local or NULL */, double* vi_sum);
/* the per-marker streaming operator on its own (src/BayesW.cpp:1499-1523): sums of vi over all
 * individuals / genotype 1 / genotype 2, with the marker's own effect taken out when beta_old != 0 */
int hgibbs_w_marker_sums(hgibbs_t h, uint32_t marker, double beta_old, double alpha, double* vi_sum, double* vi_1, double* vi_2);
/* one pass over all markers, src/BayesW.cpp:1461-1622.  rng: dist.rng (one uniform per marker);
 * ars_rng: the rand() stream; cass: G*K counts out; beta_sqnorm: G sums of squared effects out */
int hgibbs_w_sweep(hgibbs_t h, const int32_t* order_host, double alpha, const double* sigmaG, const double* pi, double sumSigmaG,
                   hgibbs_rng_state* rng, hgibbs_grand_state* ars_rng, int32_t* cass_host, double* beta_sqnorm, uint64_t* nnz_updates);
int hgibbs_w_last_sweep_stats(hgibbs_t h, hgibbs_w_sweep_stats* out);
/* diagnostic: the adaptive-rejection draw of an effect (src/BayesW.cpp:1562-1582, src/BayesW_arms.cpp:135-242) on ONE device lane,
 * `ndraws` times on the density beta_dens with the nine parameters dens9 = {alpha, sigmaG, sum_failure, sd, mean / sd, mixture value,
 * vi_0, vi_1, vi_2}, abscissae and bounds as the sweep sets them from beta_old and safe_limit: microseconds per draw (device clock),
 * density evaluations per draw, the last draw.  What the event's continuation on the device would cost. */
int hgibbs_w_ars_device_probe(hgibbs_t h, const double* dens9, double beta_old, double safe_limit, uint32_t seed, uint32_t ndraws,
                              double* us_per_draw, double* evals_per_draw, double* last_draw);
int hgibbs_w_get_beta(hgibbs_t h, double* beta, int32_t* components);
int hgibbs_w_set_beta(hgibbs_t h, const double* beta, const int32_t* components);

/* ---- BayesW chain driver: the body of BayesW::runMpiGibbs_bW (src/BayesW.cpp:905-2176) ---- */
typedef struct hydraw_chain* hydraw_chain_t;
typedef struct {
    uint32_t seed;         /* --seed: srand(seed) and dist.reset_rng(seed) (rank 0) */
    int32_t shuffle;       /* --shuf-mark */
    int32_t G, K;          /* groups; mixture components including the zero one */
    const int32_t* groups; /* M or NULL */
    const double* mS;      /* G*K, column 0 == 0 */
    int32_t quad_points;   /* --quad_points */
} hydraw_model_desc;
int hydraw_chain_create(hgibbs_t dev, const hydraw_model_desc* model, const double* y_host, const int32_t* failure_host, hydraw_chain_t* out);
int hydraw_chain_destroy(hydraw_chain_t c);
int hydraw_chain_set_covariates(hydraw_chain_t c, const double* X_host, int C);
int hydraw_chain_reseed_ars(hydraw_chain_t c, uint32_t seed);
int hydraw_chain_iterate(hydraw_chain_t c);
int hydraw_chain_state(hydraw_chain_t c, double* mu, double* alpha, double* sigmaG, double* pi, int32_t* m0, int32_t* cass,
                       hgibbs_rng_state* rng, hgibbs_grand_state* ars_rng);
int hydraw_chain_gamma(hydraw_chain_t c, double* gamma_out, int32_t* xI_out);
const int32_t* hydraw_chain_order(hydraw_chain_t c);
uint64_t hydraw_chain_last_nnz(hydraw_chain_t c);
int hydraw_chain_csv_line(hydraw_chain_t c, uint32_t iteration, char* buf, size_t len);
/* BayesW::init_from_restart (src/BayesW.cpp:869-903) + :1300-1311: the regular init, then the dumped
 * state; the ARS stream restarts at srand(ars_seed) (the reference passes opt.seed + iteration, :877) */
typedef struct {
    uint32_t iteration;
    double mu, alpha;
    const double* sigmaG;      /* G */
    const double* pi;          /* G*K */
    const double* beta;        /* M */
    const int32_t* components; /* M */
    const double* eps;         /* n_local: this rank's rows */
    const int32_t* order;      /* M */
    const double* gamma;       /* C or NULL */
    const int32_t* xI;         /* C or NULL */
    hgibbs_rng_state rng;
    uint32_t ars_seed;
} hydraw_restart_state;
int hydraw_chain_restore(hydraw_chain_t c, const hydraw_restart_state* st);

/* ---- REML heritability without the relationship matrix ---- */
/* n = the handle's rows, M_used the markers with a finite mstd, X the chain's standardisation (0 at a missing call), A = X X'/M_used.
 * Z (q x n, vector-major: column c of the design at Z + c n) holds every covariate column, the column of ones included; Q is an
 * orthonormal basis of it (modified Gram-Schmidt, twice, on the host; a dependent column is refused by its index), P_c = I - QQ',
 * H(delta) = P_c A P_c + delta I.  One rank only.  Every sum over rows or markers is taken in a fixed order (blocks of 1024 from
 * index 0, in order inside a thread, partials in block order), so each call is a deterministic function of its arguments.
 *
 * hgibbs_reml_solve: V[k] = H(delta)^-1 P_c B[k] for K <= 32 right-hand sides (B, V: K x n, vector-major) by conjugate gradients from
 * V = 0 with per-column scalars.  Column k is frozen once r'r <= tol^2 b'b (b the projected right-hand side), tested before every
 * iteration; the loop ends when every column is frozen.  iters[k] = the iterations column k took, relres[k] = sqrt(r'r / b'b) of the
 * recurrence at its end (0 for a zero column).  Reaching max_iters with a live column, or a p'Hp that is not positive and finite,
 * refuses the call. */
int hgibbs_reml_solve(hgibbs_t h, int K, int q, const double* Z, double delta, double tol, int max_iters, const double* B, double* V,
                      int* iters, double* relres);
/* hgibbs_reml_eval: the sums of f at delta from T sign probes (1 <= T <= 31) and y.  With s(c, i) = +1 when the top bit of
 * mix64((seed ^ mix64(c)) + i 0xD1B54A32D192ED03) is 0, else -1:  G_t = P_c X s(2t, marker index) / sqrt(M_used),
 * E_t = P_c s(2t + 1, row_begin + row),  b_t = G_t + sqrt(delta) E_t (t < T),  b_T = P_c y,  v_k = H^-1 b_k,  u_k = X'v_k.
 * sums[3 k + 0 .. 2] = u_k'u_k / M_used, v_k'v_k, v_k'b_k for k = 0 .. T;  f(delta) = log(sum_{t<T} vAv_t / sum_{t<T} vv_t) -
 * log(vAv_T / vv_T), the sums ascending in t.  iters (or NULL) takes the largest iteration count of the columns. */
int hgibbs_reml_eval(hgibbs_t h, int T, int q, const double* Z, const double* y, uint64_t seed, double delta, double tol, int max_iters,
                     double* sums, int* iters);
/* the root rule on x = log delta (host only).  x, f: the k >= 0 points evaluated so far.  status CONTINUE: evaluate *x_next next;
 * CONVERGED / AT_BOUND: x[k - 1] (= *x_next) is the estimate.  k = 0: log((1 - h0)/h0); k = 1: h1 = min(2 h0, (1 + h0)/2) if
 * f[0] < 0, else h0/2; then secant steps clamped to |x| <= log 9999.  Done when |x[k-1] - x[k-2]| < x_tol; the same bound twice
 * gives AT_BOUND.  f[k-1] == f[k-2], or k >= max_steps without being done, is refused. */
enum { HGIBBS_REML_CONTINUE = 0, HGIBBS_REML_CONVERGED = 1, HGIBBS_REML_AT_BOUND = 2 };
int hgibbs_reml_next(int k, const double* x, const double* f, double h0, double x_tol, int max_steps, double* x_next, int* status);
/* the estimate (host only) from the last two evaluated points x2[0], x2[1] and their sums ((T + 1) x 3 each): delta = exp(x2[1]),
 * vg = vb_T / (n - q), ve = delta vg, vp = vg + ve, h2 = 1 / (1 + delta).  ai3 (or NULL: the SEs are NaN) = a'z1, a'z2, v'z2 with
 * v = v_T, a = P_c A P_c v, H z1 = a, H z2 = v: AI = [[ai3[0], ai3[1]], [ai3[1], ai3[2]]] / (2 vg^3), the covariance of (vg, ve) is
 * its inverse and se_h2 follows by the delta method.  se_logdelta_mc: the leave-one-probe-out jackknife of the secant root through
 * the two points, sqrt((T - 1)/T sum (x_(-t) - mean)^2); se_mc = se_logdelta_mc h2 (1 - h2).  NaN when T = 1. */
typedef struct {
    double logdelta, delta, vg, ve, vp, h2;
    double se_vg, se_ve, se_vp, se_h2;
    double se_mc, se_logdelta_mc;
} hgibbs_reml_estimate;
int hgibbs_reml_finish(int T, uint32_t n, int q, const double* x2, const double* sums_prev, const double* sums_last, const double* ai3,
                       hgibbs_reml_estimate* out);
/* hgibbs_reml: the whole estimate in one call; G and E are made once and everything stays on the device across the evaluations */
#define HGIBBS_REML_MAX_STEPS 32
typedef struct {
    int trials;        /* T, 1 .. 31 */
    double h2_start;   /* h0 inside (0, 1) */
    double cg_tol;     /* positive and finite */
    int cg_iters;      /* at least 1 */
    double x_tol;      /* positive and finite */
    int max_steps;     /* 2 .. HGIBBS_REML_MAX_STEPS evaluations */
    uint64_t seed;
} hgibbs_reml_opts;
typedef struct {
    int status;        /* HGIBBS_REML_CONVERGED or HGIBBS_REML_AT_BOUND */
    int steps;         /* evaluations made */
    double x[HGIBBS_REML_MAX_STEPS], f[HGIBBS_REML_MAX_STEPS];
    int cg_iters[HGIBBS_REML_MAX_STEPS];
    double sums_prev[96], sums_last[96]; /* (T + 1) x 3 of the last two evaluations */
    double ai3[3];
    int ai_cg_iters;
    hgibbs_reml_estimate est;
    uint32_t n, m_used;
    int q, trials;
    double products_ms, algebra_ms; /* device time of the X'P and X T products, and of every other kernel */
} hgibbs_reml_result;
/* blup (or NULL): M doubles, beta_j = x_j'v_T / M_used at the estimate, NaN outside M_used */
int hgibbs_reml(hgibbs_t h, const hgibbs_reml_opts* opt, int q, const double* Z, const double* y, hgibbs_reml_result* res, double* blup);
/* device time of the last hgibbs_reml_solve / _eval / hgibbs_reml in ms: the products, the rest */
int hgibbs_last_reml_ms(hgibbs_t h, double* products_ms, double* algebra_ms);

/* ---- checkpoint / restart (src/BayesRRm.cpp:842-928, :2802-2838) --------- */
/* State a --restart run reads back from the dump files; arrays are host
 * pointers, eps has this rank's individuals.  gamma/xI may be NULL without
 * covariates.  `iteration` = the saved iteration; the chain continues at +1. */
typedef struct {
    uint32_t iteration;
    double sigmaE, mu;
    const double* sigmaG;        /* G */
    const double* estPi;         /* G*K */
    const double* beta;          /* M */
    const int32_t* components;   /* M */
    const double* eps;           /* n_local */
    const int32_t* order;        /* M: markerI as dumped in .mrk */
    const double* gamma;         /* C or NULL */
    const int32_t* xI;           /* C or NULL */
    hgibbs_rng_state rng;
} hydra_restart_state;
int hydra_chain_restore(hydra_chain_t c, const hydra_restart_state* st);
/* dist.rng in Boost's stream form (624 decimal words, `file << rng`,
 * src/distributions_boost.cpp:38-44) and back (`file >> rng`, :46-55) */
int hydra_rng_to_boost_words(const hgibbs_rng_state* st, uint32_t* words624);
int hydra_rng_from_boost_words(const uint32_t* words624, hgibbs_rng_state* st);
/* the chain's shuffle of the marker order (std::shuffle as the reference binary runs it, src/BayesRRm.cpp:1692) on a
 * caller's generator state and array: v[0..n) permuted, st advanced by the words the shuffle consumed */
int hydra_rng_shuffle(hgibbs_rng_state* st, int32_t* v, uint32_t n);
/* markers with deltaBeta != 0 in the last sweep */
uint64_t hydra_chain_last_nnz(hydra_chain_t c);

#ifdef __cplusplus
}
#endif
#endif /* HGIBBS_H */
