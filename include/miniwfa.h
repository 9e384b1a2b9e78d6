/*
 * miniwfa.h — C ABI of libmwf_hip.so, the MI355X (gfx950) implementation of miniwfa's exact
 * score-and-CIGAR path.
 *
 * PART 1 is the drop-in surface: the option/result structs and entry points of lh3/miniwfa
 * (reference miniwfa.h:32-89) with identical names, field order, sizes (56 B / 24 B), argument
 * meaning, ownership and error behaviour, so a program written against the reference header
 * links against this library unchanged.  Each declaration cites the reference line it replaces.
 *
 * PART 2 is new: a batch entry point over host buffers and a device-resident engine API
 * (plain pointers and sizes only) that the Python/torch host side and bench.py drive.
 *
 * There is no CPU fallback anywhere behind this header: every alignment runs in the HIP
 * kernels under miniwfa_amd/csrc/ (mwf_kernels.hip generic, mwf_band2.hip packed band,
 * mwf_lane.hip short pairs, mwf_mid.hip the mid-size pairs of small batches, mwf_sys.hip whole device; the reset and
 * 8-mer sketch kernels around them: mwf_sketch.hip), and every entry point aborts with a message
 * if no gfx950 device can be opened.
 */
#ifndef MWF_HIP_MINIWFA_H
#define MWF_HIP_MINIWFA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * PART 1 — drop-in surface
 * ---------------------------------------------------------------------------------------- */

/* flag bits, reference miniwfa.h:32-34 */
#define MWF_F_CIGAR      0x1      /* produce the CIGAR, not only the penalty */
#define MWF_F_NO_KALLOC  0x2      /* reference: bypass kalloc for scratch; here: accepted, no effect (scratch is device memory) */
#define MWF_F_DEBUG      0x10000  /* one line on stderr at the end of traceback (reference miniwfa.c:367) */

/* reference miniwfa.h:36-44; offsets flag@0 x@4 o1@8 e1@12 o2@16 e2@20 step@24 max_s@28 max_iter@32 max_occ@40 kmer@44 min_len@48 */
typedef struct {
	int32_t flag;
	int32_t x, o1, e1, o2, e2; /* mismatch; gap open/extend of the two affine pieces: a gap of length L costs min(o1+L*e1, o2+L*e2) */
	int32_t step;              /* >0: low-memory two-pass mode, checkpoint every `step` penalties */
	int32_t max_s;             /* >0: give up (s=-1) once the penalty exceeds this */
	int64_t max_iter;          /* >0: give up (s=-1) once more than this many (penalty,diagonal) cells were computed */
	int32_t max_occ, kmer, min_len; /* chaining heuristic only (mwf_wfa_chain) */
} mwf_opt_t;

/* reference miniwfa.h:46-51; offsets s@0 n_cigar@4 n_iter@8 cigar@16 */
typedef struct {
	int32_t s;        /* alignment penalty; -1 if stopped by max_s / max_iter */
	int32_t n_cigar;
	int64_t n_iter;   /* cells computed by the (second-pass) core loop, reference miniwfa.c:421 */
	uint32_t *cigar;  /* len<<4|op, op in {1:I, 2:D, 7:=, 8:X}; allocated from the caller's km (kfree(km,.) or free() if km==NULL) */
} mwf_rst_t;

/* reference miniwfa.h:62 / miniwfa.c:11-18: x=4 o1=4 e1=2 o2=15 e2=1 kmer=13 max_occ=2 min_len=30, rest 0 */
void mwf_opt_init(mwf_opt_t *opt);

/* reference miniwfa.h:83 / miniwfa.c:603-615: optimal global alignment of ts[0,tl) vs qs[0,ql).
 * Sequences are length-delimited arbitrary bytes compared verbatim.  *r is fully overwritten.
 * Limits of this implementation (the reference has neither; both end in a message and abort(), like the reference's
 * own assert/panic paths): max(x, o1+e1, o2+e2) < 4096 (below 256 every kernel applies; from 256 on — gap-open costs in the
 * hundreds — the pairs run on the generic kernel's big-ring form, one column per lane), and tl+ql < 2^31-4 (columns
 * are 32-bit).  x, e1, e2 >= 1 and o1, o2 >= 0, as the reference requires implicitly (miniwfa.c:390-392).
 * The fast paths hold sequences at 2 bits per base, which takes pairs of plain upper-case A/C/G/T; with "alpha_remap" (below, or MWF_ALPHA_REMAP=1 for
 * the calls that create their engines themselves) also any pair with at most four distinct bytes — lower case, U for T, bases coded 0..3.  A pair with
 * five or more distinct bytes (an N, mixed case) still runs on the byte-wise copies: one geometry of the band kernel, else the generic kernel — unless "alpha16"
 * (below, or MWF_ALPHA16=1) is set as well: under gap extensions (2,1) a pair of 5 to 16 distinct bytes then takes the band kernel's 4-bit copies (mwf_band2_nib.hip).
 * Every penalty set gives the reference's answer; which kernels serve it depends on the gap extensions (e1, e2): the whole-device kernel for
 * long pairs ("coop_min_len" below) takes (2,1), (2,2), (1,1) and e1 in {3, 4} with e2 in {1, 2} (minimap2's asm5 / asm20-like sets); under any
 * other pair of extensions long pairs run on the generic one-workgroup-per-pair kernel (about ten times slower on a 150 kb pair).  The packed
 * band kernel for big batches of mid-size pairs takes (2,1), (2,2), (1,1) and (3,1), (3,2), (4,1); under any other pair of extensions — (4,2)
 * among them, which was measured and gained too little — such batches run on the generic kernel (1.3 to 2.2 times slower on 1024 x 10 kb).
 * Under each of those six sets, pairs too long for plain 16-bit offsets (from ~6.6 kb where e2 == 2 — the -a preset's 10 kb batches —, from ~11 kb
 * where e2 == 1, up to ~21 kb) keep two workgroups per CU on that kernel's 512-thread copies on biased offsets.
 * Device: MWF_DEVICE=<ordinal> (default 0).  Any number of host threads may call concurrently. */
void mwf_wfa_exact(void *km, const mwf_opt_t *opt, int32_t tl, const char *ts, int32_t ql, const char *qs, mwf_rst_t *r);

/* reference miniwfa.h:85 / miniwfa.c:898-908: exact with step=0 and max_iter=1e8; if that stops, mwf_wfa_chain. */
void mwf_wfa_auto(void *km, const mwf_opt_t *opt, int32_t tl, const char *ts, int32_t ql, const char *qs, mwf_rst_t *r);

/* reference miniwfa.h:84 / miniwfa.c:850-896: k-mer chaining heuristic whose gap fills are exact alignments.
 * The chaining itself is host code; every gap fill runs on the device as one batch. */
void mwf_wfa_chain(void *km, const mwf_opt_t *opt, int32_t tl, const char *ts, int32_t ql, const char *qs, mwf_rst_t *r);

/* reference miniwfa.h:88-89 / mwf-dbg.c:6-31 */
int32_t mwf_cigar2score(const mwf_opt_t *opt, int32_t n_cigar, const uint32_t *cigar, int32_t *tl, int32_t *ql);
void mwf_assert_cigar(const mwf_opt_t *opt, int32_t n_cigar, const uint32_t *cigar, int32_t tl0, int32_t ql0, int32_t s0);

/* ------------------------------------------------------------------------------------------
 * PART 2 — batch and device-resident API (new; SURVEY.md §8b "New")
 * ---------------------------------------------------------------------------------------- */

/* n independent pairs from host buffers; r[i] is filled exactly as mwf_wfa_exact would fill it.  Replaces the serial
 * loop over pairs of reference main.c:67-72.  Runs on the device MWF_DEVICE names, or — when the environment sets
 * MWF_DEVICES to "all" or a count — dealt over that many devices as mwf_wfa_batch_multi does. */
void mwf_wfa_batch(void *km, const mwf_opt_t *opt, int32_t n, const int32_t *tl, const char *const *ts,
                   const int32_t *ql, const char *const *qs, mwf_rst_t *r);

/* The same over several devices of one node: pairs are dealt longest first to the device with the least
 * work so far, every device runs its share on a host thread with its own engine, nothing crosses devices while they
 * work, and the results are merged back in the caller's order.  devices: n_dev HIP ordinals (an ordinal may repeat),
 * or NULL for ordinals 0..n_dev-1 (n_dev <= 0: every visible device).  CIGARs are allocated from `km` on the calling
 * thread only. */
void mwf_wfa_batch_multi(void *km, const mwf_opt_t *opt, int32_t n, const int32_t *tl, const char *const *ts,
                         const int32_t *ql, const char *const *qs, mwf_rst_t *r, int32_t n_dev, const int32_t *devices);

/* n pairs in chain mode: r[i] is what mwf_wfa_chain would give for pair i (reference miniwfa.c:850-896 once per record, main.c:67-72).  The k-mer chaining of
 * the pairs runs on a few host threads, the gaps between the anchors of ALL pairs are aligned exactly in one device batch. */
void mwf_wfa_chain_batch(void *km, const mwf_opt_t *opt, int32_t n, const int32_t *tl, const char *const *ts,
                         const int32_t *ql, const char *const *qs, mwf_rst_t *r);

/* ... and mwf_wfa_auto of n pairs (reference miniwfa.c:898-908 once per record): the exact branch as one batch, the pairs it gives up on through mwf_wfa_chain_batch. */
void mwf_wfa_auto_batch(void *km, const mwf_opt_t *opt, int32_t n, const int32_t *tl, const char *const *ts,
                        const int32_t *ql, const char *const *qs, mwf_rst_t *r);

/* Batch throughput for callers that keep the reference's one-pair-per-call loop (reference main.c:67-72).
 * mwf_wfa_submit() queues one pair (ts / qs / *opt are read later: they must stay valid until the job has been waited for) and returns at once;
 * a dispatcher thread aligns everything submitted so far as ONE mwf_wfa_batch call per option set — while it runs, the caller may keep submitting.
 * mwf_wfa_wait() blocks until the job is done, fills *r exactly as mwf_wfa_exact would (CIGAR allocated from `km` on the waiting thread) and
 * frees the job.  A pair waits at most MWF_COALESCE_US microseconds (default 100) for company unless a wait arrives first.
 * MWF_COALESCE_US=n (n > 0) in the environment also routes plain mwf_wfa_exact calls through the same dispatcher: calls from different host
 * threads that arrive within n microseconds share one launch (opt-in: a lone caller pays up to n microseconds per call). */
typedef struct mwf_job_s mwf_job_t;
mwf_job_t *mwf_wfa_submit(const mwf_opt_t *opt, int32_t tl, const char *ts, int32_t ql, const char *qs);
void mwf_wfa_wait(void *km, mwf_job_t *job, mwf_rst_t *r);
/* diagnostics: batches the dispatcher has run so far, pairs in them */
void mwf_wfa_async_stats(int64_t *n_batches, int64_t *n_jobs);

typedef struct mwf_gpu_s mwf_gpu_t;             /* engine: one device, one stream, one memory pool */
typedef struct mwf_gpu_batch_s mwf_gpu_batch_t; /* a set of pairs resident in that device's HBM */

int         mwf_gpu_device_count(void);
/* device: HIP ordinal.  stream: a hipStream_t to enqueue on, or NULL to let the engine create its own. */
mwf_gpu_t  *mwf_gpu_create(int device, void *stream);
void        mwf_gpu_destroy(mwf_gpu_t *g);
const char *mwf_gpu_last_error(const mwf_gpu_t *g);

/* Packed layout: all sequences back to back in `seqs` (seq_bytes bytes, +>=16 readable bytes of slack);
 * pair i is target seqs[t_off[i], t_off[i]+tl[i]) and query seqs[q_off[i], q_off[i]+ql[i]).
 * _upload copies from host memory; _wrap adopts buffers that already live in this device's HBM
 * (e.g. torch tensors) without copying — they must outlive the batch object. */
mwf_gpu_batch_t *mwf_gpu_batch_upload(mwf_gpu_t *g, int32_t n, const char *seqs, int64_t seq_bytes,
                                      const int64_t *t_off, const int32_t *tl, const int64_t *q_off, const int32_t *ql);
mwf_gpu_batch_t *mwf_gpu_batch_wrap(mwf_gpu_t *g, int32_t n, const void *d_seqs, int64_t seq_bytes,
                                    const int64_t *d_t_off, const int32_t *d_tl, const int64_t *d_q_off, const int32_t *d_ql,
                                    const int32_t *h_tl, const int32_t *h_ql);
void mwf_gpu_batch_free(mwf_gpu_batch_t *b);

/* Align every pair of the batch with `opt`.  Kernels are enqueued on the engine's stream; the call
 * returns after they are enqueued — except on the whole-device kernel (a few long pairs), whose launches are serialised
 * per device and waited for.  Pairs that need a re-run get it in mwf_gpu_batch_results().  Returns 0, or a negative
 * error (see mwf_gpu_last_error).
 * The first align of a batch (and the first after its options or the engine's tunables change) plans it: in a batch of
 * more long pairs than the device holds at once it also reads every pair's sequences for an 8-mer work estimate (one small
 * kernel and one wait) and deals the pairs by it.  That order is a scheduling hint kept with the plan: if a wrapped
 * batch's contents change later, it costs speed, never correctness. */
int mwf_gpu_batch_align(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt);

/* Wait for the batch and copy the fixed-size results to host arrays of length n (any may be NULL). */
int mwf_gpu_batch_results(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t *s, int64_t *n_iter, int32_t *n_cigar);
/* Device pointers to the same fixed-size results (int32 s[n], int64 n_iter[n], int32 status[n]) for zero-copy consumers.
 * They are FINAL only after mwf_gpu_batch_results() returned: a pair whose window or traceback outgrew the workspace of
 * the kernel it ran on is re-run by that call.  Until then such a pair reads s == -2 (never a valid answer; -1 means
 * "stopped by max_s / max_iter", as in the reference) and status != 0 (0: done, 1: stopped). */
const int32_t *mwf_gpu_batch_dev_scores(const mwf_gpu_batch_t *b);
const int64_t *mwf_gpu_batch_dev_iters(const mwf_gpu_batch_t *b);
const int32_t *mwf_gpu_batch_dev_status(const mwf_gpu_batch_t *b);
/* CIGAR of pair i into dst (capacity cap words); returns n_cigar or a negative error. */
int32_t mwf_gpu_batch_cigar(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t i, uint32_t *dst, int32_t cap);
/* Optional: bring every CIGAR of the batch to the host in one copy; mwf_gpu_batch_cigar then serves from that copy. */
int mwf_gpu_batch_fetch_cigars(mwf_gpu_t *g, mwf_gpu_batch_t *b);

/* ---- After the align: summaries, CIGAR checks and coordinate maps without leaving the device (kernels: csrc/mwf_cigar_ops.hip) ---- */

/* What a CIGAR says about its pair, and whether it is an alignment of THESE sequences: the counters a caller derives identity and
 * gap statistics from, plus the self-check the reference's CLI runs on every record (mwf_assert_cigar) extended to the bases. */
typedef struct {            /* 48 bytes, twelve int32 */
	int32_t score;          /* what mwf_cigar2score gives for the words under the options used */
	int32_t t_len, q_len;   /* bases of target / query the words consume */
	int32_t n_eq, n_x;      /* bases under '=' / 'X' */
	int32_t n_ins, n_del;   /* bases under 'I' (query only) / 'D' (target only) */
	int32_t n_ins_runs, n_del_runs; /* words with op I / D (each pays one gap open in `score`) */
	int32_t n_words;        /* words summarised */
	int32_t first_bad;      /* -1: the words are a valid alignment of THESE sequences; else see below */
	int32_t flags;          /* bit 0: the pair has a CIGAR (otherwise every other field is 0 and first_bad is -1); other bits 0 */
} mwf_aln_summary_t;
/* first_bad: walk the words in order with running start positions (ti, qj), kept in 64 bits; every word with a known op (1 I, 2 D,
 * 7 =, 8 X) advances them by its full length, whatever else is wrong with it.  Word w is bad if (a) its op is none of those four
 * (such a word consumes nothing and counts nowhere), or (b) it runs past the end of a sequence (ti+len > tl for D, = and X; qj+len > ql
 * for I, = and X), or (c) it is = or X and some base of its in-range part contradicts the op (t[ti+k] != q[qj+k] under =, equal under X,
 * for k < min(len, tl-ti, ql-qj)).  first_bad is the smallest bad w; without one it is n_words if (ti, qj) != (tl, ql), else -1.
 * score and the counters accumulate in 64 bits from the full word lengths and are truncated on store. */

/* The host twin: the summary of one CIGAR against one pair of sequences.  Needs no device.  Never reads outside ts[0,tl) / qs[0,ql),
 * whatever the words say.  flags is always 1 here (n_cigar == 0 is an empty CIGAR: first_bad 0 unless both sequences are empty). */
void mwf_cigar_summary(const mwf_opt_t *opt, int32_t n_cigar, const uint32_t *cigar, int32_t tl, const char *ts, int32_t ql, const char *qs,
                       mwf_aln_summary_t *out);

/* Zero-copy access to the CIGARs of the batch's last CIGAR-mode align: finalises the batch as mwf_gpu_batch_results() does, then hands out
 * device pointers: pair i's words are pool[word_off[i] .. word_off[i] + n_words[i]).  The pool is unordered and has holes: only word_off
 * and n_words address it; *pool_words is how many words from `pool` on are in use (holes included).  Valid until the next align or free
 * of the batch.  Any output pointer may be NULL.  Fails (negative; mwf_gpu_last_error) if the last align was score-only. */
int mwf_gpu_batch_dev_cigars(mwf_gpu_t *g, mwf_gpu_batch_t *b, const uint32_t **pool, const int64_t **word_off, const int32_t **n_words, int64_t *pool_words);

/* Enqueue the summary kernel on the engine's stream: one mwf_aln_summary_t per pair into a library-owned device array; returns without
 * waiting for the kernel.  opt == NULL: the options of the last align (only x, o1, e1, o2, e2 are used).
 * d_words, d_word_off, d_n_words all NULL: the batch's own CIGARs — the call finalises the batch first (and waits for that), a pair has a
 * CIGAR when its status is 0 (a stopped pair's record has flags == 0), and the call fails if the last align was score-only.
 * Otherwise all three are caller-owned device arrays: foreign CIGARs for the batch's sequences (stitched chain-mode CIGARs, another
 * aligner's), pair i's words at d_words[d_word_off[i] .. + d_n_words[i]); they are trusted only to lie inside the caller's allocation —
 * malformed words yield a record (first_bad), never a read outside a pair's sequences.  A pair with d_n_words[i] <= 0 has no CIGAR.
 * Work the caller enqueued on other streams (the tensors' producer) must be complete. */
int mwf_gpu_batch_summarize(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const uint32_t *d_words, const int64_t *d_word_off, const int32_t *d_n_words);
/* Device pointer to the n records of the last summarize; NULL before the first one and after a newer align made them stale. */
const mwf_aln_summary_t *mwf_gpu_batch_dev_summary(const mwf_gpu_batch_t *b);
/* Wait and copy the n records to host_out. */
int mwf_gpu_batch_summary(mwf_gpu_t *g, mwf_gpu_batch_t *b, mwf_aln_summary_t *host_out);

/* Coordinate maps of the batch's own CIGARs (finalises; fails after a score-only align).  which 0: query -> target, 1: target -> query.
 * A map is a dense int32 array in pair order: pair i occupies [off[i], off[i] + ql[i]) (which 0) or [off[i], off[i] + tl[i]) (which 1),
 * off = exclusive prefix sum of those lengths.  A base under = or X holds the index of its partner; a query base under I holds
 * -1 - t_next, t_next in 0 .. tl being the next target base to be consumed (a target base under D: -1 - q_next); every position of a pair
 * without a CIGAR (stopped, s == -1) holds INT32_MIN.  Writes are clipped to the pair's range.  _map enqueues the kernel and returns. */
int mwf_gpu_batch_map(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t which);
/* Device pointer to that map; NULL before the first mwf_gpu_batch_map(.., which) and after a newer align. */
const int32_t *mwf_gpu_batch_dev_map(const mwf_gpu_batch_t *b, int32_t which);
/* Wait and copy the map to host_out (sum of the lengths int32) and, unless NULL, its n + 1 offsets to host_off. */
int mwf_gpu_batch_map_fetch(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t which, int32_t *host_out, int64_t *host_off);
/* The summary array and the maps are allocated on first use through the engine's accounting (mwf_gpu_stats_t dev_bytes / dev_bytes_peak
 * include them while the batch lives) and freed with the batch; a caller that never asks pays nothing. */

/* ---- Alignment text: the form in which an alignment leaves a mapper (kernels: csrc/mwf_cigar_text.hip) ---- */

/* The six products (`kind`).  The target plays SAM's reference. */
#define MWF_TXT_CIGAR 0 /* the CIGAR as the reference's CLI prints it */
#define MWF_TXT_SAM   1 /* SAM's M-form */
#define MWF_TXT_CS    2 /* minimap2's cs tag (short form) */
#define MWF_TXT_MD    3 /* SAM's MD tag */
#define MWF_TXT_ROW_T 4 /* the gapped target row */
#define MWF_TXT_ROW_Q 5 /* the gapped query row */
#define MWF_TXT_KINDS 6
/* Renderable: words are renderable for a pair iff every op is one of 1 I, 2 D, 7 =, 8 X, every length is >= 1, no word runs past a sequence
 * (rules (a) and (b) of first_bad above) and the words end exactly at (tl, ql).  Bases under = and X are not compared (that is summarize's job).
 * Decimal numbers have no leading zeros and no sign; sums are formed in 64 bits.  No terminators, no separators.
 *   0 CIGAR  per word <len><c>, c = "MIDNSHP=X"[op]
 *   1 SAM    a maximal run of consecutive words with op = or X becomes one <sum>M; I and D words are printed per word and never merged
 *   2 cs     per word: = gives :<len>; X gives *<t><q> for each base; I gives + and the query bases; D gives - and the target bases.  Bytes
 *            'A'..'Z' are lowered (b | 0x20), every other byte is copied verbatim
 *   3 MD     a running count c of bases under =.  Every base under X: c (also when it is 0), the target byte verbatim, c = 0.  Every D word:
 *            c, '^', its target bytes verbatim, c = 0.  I words are invisible (c runs across them).  At the end: c — a pair of two empty
 *            sequences (no words) has the MD "0"
 *   4, 5 rows  one byte per alignment column in word order, bytes verbatim; the target row (4) has '-' under I, the query row (5) '-' under
 *            D; both are n_eq + n_x + n_ins + n_del bytes long
 * 10= 1X 3D 8= 2I 12= on ACGTTGCAACGCATGGATCCTACGATCGGATTAC / ACGTTGCAACTGGATCCTATTCGATCGGATTAC:  10=1X3D8=2I12=  11M3D8M2I12M
 * :10*gt-cat:8+tt:12  10G0^CAT20  ACGTTGCAACGCATGGATCCTA--CGATCGGATTAC  ACGTTGCAACT---GGATCCTATTCGATCGGATTAC */

/* The host twin: text `kind` of one CIGAR against one pair.  Returns the full length of the text, snprintf-style (it may exceed cap); at most
 * cap bytes are written; dst may be NULL when cap is 0.  Returns -1 and writes nothing when the words are not renderable or kind is out of
 * range.  Needs no device.  Never reads outside ts[0,tl) / qs[0,ql), whatever the words say. */
int64_t mwf_cigar_text(int32_t kind, int32_t n_cigar, const uint32_t *cigar, int32_t tl, const char *ts, int32_t ql, const char *qs,
                       char *dst, int64_t cap);

/* The device form: text `kind` of every pair into a library-owned pool, pair i's text at txt[off[i] .. off[i + 1]), off int64[n + 1] on the
 * device.  A sizing launch, a device-side scan into off, one host wait for the total, the pool's allocation, then the writing launch is
 * enqueued and the call returns.  d_words, d_word_off, d_n_words all NULL: the batch's own CIGARs (finalises; fails after a score-only
 * align); otherwise foreign device arrays for the batch's sequences under the trust rules of mwf_gpu_batch_summarize.  Stopped pairs
 * (status != 0), foreign pairs with d_n_words[i] <= 0 and pairs whose words are not renderable get empty text (off[i] == off[i + 1]; their MD
 * is empty too); unrenderable words never cause an access outside the pair's sequences or its slice of the pool. */
int mwf_gpu_batch_text(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t kind, const uint32_t *d_words, const int64_t *d_word_off, const int32_t *d_n_words);
/* Device pointer to that text, its n + 1 offsets and the total bytes (d_off / total may be NULL); NULL before the first mwf_gpu_batch_text(.., kind, ..)
 * and after a newer align.  One pool per kind, counted in dev_bytes / dev_bytes_peak, freed with the batch. */
const char *mwf_gpu_batch_dev_text(const mwf_gpu_batch_t *b, int32_t kind, const int64_t **d_off, int64_t *total);
/* Wait and copy the text (total bytes) to host_out and its n + 1 offsets to host_off (either may be NULL). */
int mwf_gpu_batch_text_fetch(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t kind, char *host_out, int64_t *host_off);

/* ---- Alphabet classes (kernels: csrc/mwf_alphabet.hip) ---- */

/* The class of one pair by the bytes that occur in target and query together: 0 every byte is one of A C G T (upper case; two empty sequences
 * included), 1 at most four distinct bytes and not class 0, 2 five or more.  The alignment only needs the equality relation between bytes, so a
 * class-1 pair can be aligned as a plain one after a bijection of its bytes: the distinct bytes in ascending byte value map to 'A', 'C', 'G', 'T'
 * in that order.  map (256 bytes; may be NULL): for class 1, map[b] is that letter for every byte b that occurs and 0 for every other; for classes
 * 0 and 2 all 256 entries are 0.  Needs no device.  Never reads outside ts[0,tl) / qs[0,ql). */
int32_t mwf_alphabet_class(int32_t tl, const char *ts, int32_t ql, const char *qs, uint8_t map[256]);

/* The same with one class more, as the engine sees a pair under "alpha16" 1: 0 and 1 as above, 3 five to sixteen distinct bytes, 2 seventeen or more.  A class-3
 * pair can be aligned as its image under the bijection that gives the distinct bytes, in ascending byte value, the codes 0 ... 15: the image byte is
 * MWF_ALPHA16_TAG | code.  map: for class 1 as mwf_alphabet_class gives it; for class 3 the image byte of every byte that occurs, 0 elsewhere; all zero for
 * classes 0 and 2.  Needs no device.  Never reads outside ts[0,tl) / qs[0,ql). */
#define MWF_ALPHA16_TAG 0x40 /* the fixed high nibble of a class-3 image byte */
int32_t mwf_alphabet_class16(int32_t tl, const char *ts, int32_t ql, const char *qs, uint8_t map[256]);

/* Per-pair class (0, 1, 2 as above; with "alpha16" 1: 0, 1, 2, 3 as mwf_alphabet_class16) of the batch's last align under "alpha_remap" 1, copied to host_out[n].  Fails (negative; mwf_gpu_last_error)
 * before the first align and when that align ran with the tunable off. */
int mwf_gpu_batch_alphabet(mwf_gpu_t *g, mwf_gpu_batch_t *b, int8_t *host_out);

/* ---- Ends-free (semi-global) alignment (kernel: csrc/mwf_ends.hip) ---- */

/* Every other call here aligns both sequences end to end.  A caller behind a mapper holds a window around a seed hit, not the interval a read
 * aligns to; an ends-free alignment leaves bases at the ends of the sequences unaligned at no cost, up to four allowances.
 *
 * Allowances.  Each is the largest number of bases that may be left unaligned, free of charge, at the begin or the end of the target or the query.
 * Each must be >= 0 and is clamped to that sequence's length; one set applies to every pair of a batch (one per pair: mwf_gpu_batch_align_ends_pp below).  The usual sets:
 * read in window {INT32_MAX, INT32_MAX, 0, 0}; extension from an anchor {0, INT32_MAX, 0, INT32_MAX}; overlap {0, INT32_MAX, longest overhang, 0} and its mirror
 * (penalties only: with t_end and q_beg — or t_beg and q_end — both unbounded the empty alignment in that corner of the matrix costs nothing and always wins).
 *
 * The result is the cheapest global alignment, under opt's two-piece affine penalties, of t[tb, te) against q[qb, qe) where
 *   - at most one of tb, qb is non-zero: tb <= t_beg with qb == 0, or qb <= q_beg with tb == 0;
 *   - te == tl or qe == ql, with tl - te <= t_end and ql - qe <= q_end.
 *
 * How it is found (conventions: diagonal d = i - k, query index minus target index, in column d + tl + 1; an H value k is the index of the last target
 * base consumed, i = d + k that of the last query base):
 *   Penalty 0.  The window is the diagonals [-min(t_beg, tl), min(q_beg, ql)]; H[d] = (d < 0 ? -d : 0) - 1, then extended along matches; E and F are dead.
 *   End rule.  Evaluated on every in-matrix H cell after its extension, penalty 0 included: cell (d, k) ends the alignment if i == ql-1 && tl-1-k <= t_end,
 *   or k == tl-1 && ql-1-i <= q_end.  The answer is the first penalty that has such a cell; among several the lowest diagonal (the order of the reference's
 *   sweep).  te = k + 1, qe = i + 1.  The traceback starts there, in the state of the cell's low three traceback bits if the extension did not move it, else 0.
 *   Band bookkeeping and n_iter are those of the global pass: growth by one column per side, clamped to [1, tl+ql+1]; the edge rule; the shrink at every
 *   multiple of 256; n_iter += hi-lo+1 per penalty from 1 on; the max_s / max_iter stop rules.  With four zero allowances s, n_iter and the CIGAR words are
 *   therefore those of mwf_gpu_batch_align / mwf_wfa_exact.
 *   Traceback.  The walk leaves the matrix with either i >= 0 query bases or k >= 0 target bases still in front of it.  With L that count,
 *   clip = min(L, begin allowance of that sequence) bases are clipped — qb or tb — and the remaining L - clip are one I (query) or D (target) run, merged with
 *   an adjacent run of the same operation.  The CIGAR holds only = X I D words for the aligned ranges: no clip operators.
 *
 * Outputs.  Per pair range[4] = {tb, te, qb, qe}, half-open.  A stopped pair (max_s / max_iter) has s == -1 and all four -1; a score-only align fills te and
 * qe and leaves tb = qb = -1.  An empty alignment is legal (n_cigar == 0, tb == te). */
typedef struct { int32_t t_beg, t_end, q_beg, q_end; } mwf_ends_t; /* 16 bytes */

/* mwf_gpu_batch_align for an ends-free alignment: validates as it does, and also returns -2 (mwf_gpu_last_error) for a negative allowance, for
 * MWF_F_CIGAR together with opt->step > 0 (no low-memory mode) and for max(x, o1+e1, o2+e2) >= 256.  One launch of the ends-free kernel over all pairs,
 * longest first; always on the batch's original bytes ("alpha_remap" / "alpha16" do not apply).  mwf_gpu_get_stats reports kernel_kind 3.  Results, CIGARs,
 * mwf_gpu_batch_summarize and mwf_gpu_batch_text work as after mwf_gpu_batch_align — summaries and text of the batch's own CIGARs describe the aligned
 * sub-ranges t[tb, te) / q[qb, qe), foreign CIGARs the full sequences —; mwf_gpu_batch_map fails after an ends-free align.  A later mwf_gpu_batch_align on
 * the same batch behaves as if this call had never been made. */
int mwf_gpu_batch_align_ends(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ends_t *ends);
/* The ranges of the last ends-free align, copied to range[n * 4]; waits for the stream.  Fails (negative) when the batch's last align was a plain one. */
int mwf_gpu_batch_ranges(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t *range);
/* ... and the device array they lie in (n x 4 int32; complete once the batch is finalised, e.g. by mwf_gpu_batch_results); NULL after a plain align. */
const int32_t *mwf_gpu_batch_dev_ranges(const mwf_gpu_batch_t *b);

/* The host-buffer calls, on pooled engines as mwf_wfa_batch: r as mwf_wfa_exact fills it, range[4] (one pair) / range[n * 4] may be NULL. */
void mwf_wfa_ends(void *km, const mwf_opt_t *opt, const mwf_ends_t *ends, int32_t tl, const char *ts, int32_t ql, const char *qs, mwf_rst_t *r, int32_t *range);
void mwf_wfa_ends_batch(void *km, const mwf_opt_t *opt, const mwf_ends_t *ends, int32_t n, const int32_t *tl, const char *const *ts,
                        const int32_t *ql, const char *const *qs, mwf_rst_t *r, int32_t *range);

/* ---- Extension alignment: the best-scoring prefix, with a drop-off stop (kernel: csrc/mwf_ends.hip, its EXT form) ---- */

/* Outside a mapper's outermost anchors an alignment is extended from the anchor outwards and stops where it stops being worth it.  The ends-free
 * allowances {0, INT32_MAX, 0, INT32_MAX} run until one sequence is used up — penalties alone never reward a match — and so force an adapter, a
 * chimeric tail or a low-quality end into the alignment.  An extension alignment scores every cell of that same pass and answers the best one.
 *
 * Parameters, one set per batch: match = A >= 1; zdrop = Z >= 0, or -1 for "no drop rule".
 *
 * The pass is the ends-free pass (mwf_ends_t above) with the allowances fixed at {0, INT32_MAX, 0, INT32_MAX}: a single origin cell on diagonal 0, the
 * same conventions (column = diagonal + tl + 1, an H value k is the last target base consumed, i = d + k), the same band bookkeeping, n_iter and
 * max_s / max_iter stop rules.  An H cell that is tested after its extension at penalty s has consumed a = (i+1) + (k+1) = d + 2k + 2 bases of the
 * two sequences together (the origin cell at penalty 0 is a candidate even when it consumes nothing), and its score is
 *     V = A * a - 2 * s,
 * twice the score of the cell's alignment under the scheme: match +A, mismatch -(x - A), a gap of L bases -(o + L * (e - A/2)).  A = 1 with the
 * default penalties (x 4, o1 4, e1 2, o2 15, e2 1) is therefore a 1 / -3 / -4 / -1.5 scheme (second piece -15 / -0.5).  A >= 2 * min(e1, e2)
 * rewards gaps: legal, but pointless.
 *
 * Per penalty s that has at least one such cell:
 *   1. a_s = the largest a among them (s is constant within a penalty, so the penalty's best V is A * a_s - 2 s); among equal a the lowest column wins.
 *   2. If A * a_s - 2 s is strictly greater than the best so far, B, it becomes B and its cell (penalty, column, offset, start state) the answer so
 *      far.  An equal V at a later penalty does not replace it.
 *   3. F = max(F, a_s): the furthest anti-diagonal any penalty so far has reached.  A * F - 2 s bounds the V of every cell at penalty s from above,
 *      and falls by 2 per penalty while the frontier stands still.
 *   4. The pass ends, tested after steps 1-3 of the same penalty, on
 *        end  (MWF_EXT_END):  some tested cell has i == ql-1 or k == tl-1 (the ends-free end rule with unbounded end allowances), or
 *        drop (MWF_EXT_DROP): Z >= 0 and B - (A * F - 2 s) > Z;  a penalty at which both hold reports end.
 *      The max_s / max_iter rules come first, as in every pass: such a pair is stopped (s == -1, ranges and info all -1).
 * Penalties with no in-matrix H cell leave B and F alone; the drop test still runs for them.  (Under two-piece penalties many penalties are
 * unreachable or hold only laggard cells: that is why the drop is measured against the monotone F and not against the penalty's own maximum.)
 *
 * The result is the remembered cell: s its penalty; te = k+1, qe = i+1, tb = qb = 0 (the ranges are complete in score-only mode too); the CIGAR is
 * the ends-free traceback started at that cell, in the state of its low three traceback bits if the extension did not move it, else 0; n_iter counts
 * the whole pass up to the stop.  An empty alignment is legal: te = qe = 0, n_cigar = 0, V = 0.  Per pair info[4] = {V, s_stop, why, F}: s_stop the
 * penalty at which the pass ended.  Extending to the left of an anchor is extending the two reversed sequences: the caller reverses them. */
typedef struct { int32_t match, zdrop; } mwf_ext_t; /* 8 bytes */
#define MWF_EXT_END  0
#define MWF_EXT_DROP 1

/* mwf_gpu_batch_align_ends under the extension rule.  Refuses (-2, mwf_gpu_last_error) what that call refuses and also match < 1, zdrop < -1 and a pair
 * with match * (tl+ql+2) >= 2^31 or tl+ql+2 >= 2^30.  Afterwards the batch behaves as after an ends-free align: mwf_gpu_batch_ranges, results, CIGARs,
 * mwf_gpu_batch_summarize and mwf_gpu_batch_text (of the sub-ranges t[0, te) / q[0, qe)) work, mwf_gpu_batch_map fails, kernel_kind is 3; a traceback arena
 * that was too small is met by the same re-run, under the same rule.  A later mwf_gpu_batch_align or mwf_gpu_batch_align_ends on the same batch behaves as
 * if this call had never been made. */
int mwf_gpu_batch_align_ext(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ext_t *ext);
/* info of the last extension align, copied to info[n * 4]; waits for the stream.  Fails (negative) when the batch's last align was not an extension. */
int mwf_gpu_batch_ext_info(mwf_gpu_t *g, mwf_gpu_batch_t *b, int32_t *info);
/* ... and the device array it lies in (n x 4 int32; complete once the batch is finalised); NULL after any other align. */
const int32_t *mwf_gpu_batch_dev_ext_info(const mwf_gpu_batch_t *b);

/* The host-buffer calls, as mwf_wfa_ends / mwf_wfa_ends_batch: range[4] and info[4] (one pair) / range[n * 4] and info[n * 4] may be NULL. */
void mwf_wfa_ext(void *km, const mwf_opt_t *opt, const mwf_ext_t *ext, int32_t tl, const char *ts, int32_t ql, const char *qs, mwf_rst_t *r, int32_t *range, int32_t *info);
void mwf_wfa_ext_batch(void *km, const mwf_opt_t *opt, const mwf_ext_t *ext, int32_t n, const int32_t *tl, const char *const *ts,
                       const int32_t *ql, const char *const *qs, mwf_rst_t *r, int32_t *range, int32_t *info);

/* ---- Per-pair allowances and diagonal bands for the two alignments above (same kernels: csrc/mwf_ends.hip) ---- */

/* A mapper has, for every read, a window with its own slack, an overlap with its own overhang, and a seed diagonal the alignment should stay near.
 *
 * Per-pair allowances.  ends[i] is pair i's mwf_ends_t, with the meaning and the clamping stated above; n_ends == 1 gives one set to every pair.
 *
 * Band.  band[i] = {d_lo, d_hi} is an inclusive range of diagonals, d = query index - target index as everywhere in this header; from a seed at
 * (t_pos, q_pos) and a bandwidth bw it is {q_pos - t_pos - bw, q_pos - t_pos + bw}.  It is clamped on the device to the diagonals the matrix has,
 * [-tl, ql]; any int32 values are legal, and d_lo > d_hi admits nothing.  The answer is the cheapest alignment the allowances permit (for an extension:
 * the best-scoring cell) among alignments whose EVERY cell lies on a diagonal inside the band — H, E1, F1, E2 and F2 alike: a gap moves one diagonal per
 * base, so a gap may not leave the band either.
 *
 * How it is found: the pass stated above with two clamps.  In columns (diagonal + tl + 1) the clamped band is [blo, bhi];
 *   Origin.  The window of penalty 0 is intersected with [blo, bhi].
 *   Growth.  Each new slice is lo = max(wf_lo - 1, 1, blo), hi = min(wf_hi + 1, tl+ql+1, bhi).
 * Everything else applies to the clamped windows as written: the edge rule, the shrink at multiples of 256, n_iter += hi-lo+1, the stop rules, the end
 * rule, the extension rule with B, F and the drop test, the traceback and its clipping (by the pair's own begin allowances).  With no band, or a band
 * that covers [-tl, ql], s, n_iter, ranges, info and CIGAR words are bit for bit those of mwf_gpu_batch_align_ends / mwf_gpu_batch_align_ext.
 *
 * Feasibility.  With the allowances clamped to the lengths, an alignment begins on a diagonal of [-t_beg, q_beg] and ends on one of
 * [ql - tl - q_end, ql - tl + t_end].  An alignment inside the band exists iff the clamped band is non-empty and meets both intervals; for an extension
 * that is d_lo <= 0 <= d_hi.  A pair whose band admits no alignment is an answer, not an error — one read with a bad seed does not fail a batch —: the
 * kernel tests the rule at the start of the pair and writes the stopped record, s == -1, n_iter == 0, n_cigar == 0, ranges and info all -1.
 * s == -1 with n_iter == 0 therefore means "nothing inside the band"; a max_s / max_iter stop always has n_iter >= 1.
 *
 * Penalty bound.  gap(tl) + gap(ql) — delete the target, insert the query — leaves the band and does not bound a banded alignment (two unrelated
 * 100-base sequences under the band {0, 0} cost 400 with the default penalties).  Inside any feasible band lies a path of diagonal steps and one gap:
 * s <= x * min(tl, ql) + max(gap(tl), gap(ql)).  The workspace of a banded launch is sized by that bound. */
typedef struct { int32_t d_lo, d_hi; } mwf_band_t; /* 8 bytes, inclusive diagonals */

/* mwf_gpu_batch_align_ends with per-pair parameters.  ends: n_ends host entries, n_ends == 1 (one set for all pairs) or n_ends == n; band: n host
 * entries, or NULL for no band.  Both are copied before the call returns.  Refuses (-2, mwf_gpu_last_error) what mwf_gpu_batch_align_ends refuses and
 * also n_ends outside {1, n} and a negative allowance of any pair (the message names the first such pair).  Afterwards the batch behaves as after
 * mwf_gpu_batch_align_ends (ranges, results, CIGARs, summaries and text of the sub-ranges; mwf_gpu_batch_map fails; kernel_kind 3), and a re-run of
 * pairs whose traceback arena was too small repeats the same per-pair parameters.  A later mwf_gpu_batch_align, _align_ends or _align_ext on the same
 * batch behaves as if this call had never been made: neither the allowances nor the band stay. */
int mwf_gpu_batch_align_ends_pp(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ends_t *ends, int32_t n_ends, const mwf_band_t *band);
/* mwf_gpu_batch_align_ext under a per-pair band (band: n host entries, not NULL): refuses what that call refuses; afterwards as after it. */
int mwf_gpu_batch_align_ext_band(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ext_t *ext, const mwf_band_t *band);

/* The host-buffer calls, on pooled engines as mwf_wfa_ends_batch / mwf_wfa_ext_batch: ends[n_ends] and band[n] (or NULL) / band[n] describe the n pairs. */
void mwf_wfa_ends_pp_batch(void *km, const mwf_opt_t *opt, const mwf_ends_t *ends, int32_t n_ends, const mwf_band_t *band, int32_t n, const int32_t *tl, const char *const *ts,
                           const int32_t *ql, const char *const *qs, mwf_rst_t *r, int32_t *range);
void mwf_wfa_ext_band_batch(void *km, const mwf_opt_t *opt, const mwf_ext_t *ext, const mwf_band_t *band, int32_t n, const int32_t *tl, const char *const *ts,
                            const int32_t *ql, const char *const *qs, mwf_rst_t *r, int32_t *range, int32_t *info);

/* Timing and counters of the most recent mwf_gpu_batch_align on this engine. */
typedef struct {
	double  kernel_ms;     /* HIP-event time around the alignment kernels on the engine's stream */
	int64_t cells;         /* (penalty,diagonal) cells computed by core passes (= sum of n_iter) */
	int64_t cells_pass1;   /* cells computed by low-memory first passes (not part of n_iter) */
	int32_t n_launches;    /* kernel launches issued */
	int32_t n_retries;     /* re-runs of pairs the kernel they ran on handed back, all causes counted: window beyond the kernel's span, 16-bit offset range, a base outside A/C/G/T, traceback arena, CIGAR pool (a pair can be re-run more than once) */
	int32_t grid, block;   /* geometry of the dominant launch */
	int32_t kernel_kind;   /* 0: one workgroup per pair (generic); 1: one pair across the whole device; 2: one workgroup per pair (band); 3: one workgroup per pair (ends-free, mwf_gpu_batch_align_ends) */
	int64_t dev_bytes;     /* device memory the engine holds now: workspace pools + recycled batch allocations (live batches hold their own) */
	int64_t dev_bytes_peak;/* ... and the most it held since creation or the last mwf_gpu_set(g, "trim", 0) */
	int32_t packed;        /* band kernels: 1 = the packed 16-bit variant (mwf_band2.hip; with block 1024: its span geometry for pairs of up to ~60 kb), 32 = the one-wave-per-pair lane kernel (mwf_lane.hip), 33 = the one-workgroup-per-pair mid kernel (mwf_mid.hip); generic kernel: 16 = 16-bit ring rows */
	int32_t lowmem_two_pass; /* low-memory mode: 1 = the first pass stored no traceback (provenance + snapshots), 0 = checkpoints walked off a full traceback */
} mwf_gpu_stats_t;
void mwf_gpu_get_stats(const mwf_gpu_t *g, mwf_gpu_stats_t *st);

/* Diagnostics: align with `opt` and report the column window [lo,hi] (column = diagonal + tl + 1) of every
 * wavefront slice the core pass opened for `pair`; returns the number of penalties written (<= cap). */
int32_t mwf_gpu_debug_band(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, int32_t pair, int32_t *lohi, int32_t cap);

/* Tunables (call before align; every call invalidates the cached plans of the engine's batches).  Sixteen names and one action:
 *   "tb_budget_mb"      traceback arena of the one-workgroup-per-pair kernels (0 = automatic: four fifths of what is free, at most a quarter of the device)
 *   "lowmem_budget_mb"  whole-device kernel, opt.step > 0: a first-pass traceback above this many MB switches to the two-pass form whose first pass stores none (0 = a quarter of the device)
 *   "coop_min_len"      tl + ql from which a batch of at most sixteen pairs runs on the whole-device kernel (0 = 20 000 score-only, 15 000 with CIGAR);
 *                       applies to the gap extensions that kernel is built for — (2,1), (2,2), (1,1), (3,1), (3,2), (4,1), (4,2) —, others stay on the generic kernel
 *   "seq2bit"           1 (default): pairs of plain A/C/G/T are held at 2 bits per base in LDS, any other pair runs on the byte-wise copy; 0: always bytes
 *   "ring16"            generic kernel: 1 (default) = 16-bit ring rows while target length + penalty fits 16 bits (half the HBM traffic); 0: always 32-bit rows
 *   "band_span"         1 (default): pairs beyond the 512-thread geometry (to 62 000 bases per sequence, windows to ~20 000 columns) run on the packed kernel's
 *                       1024-thread span geometry instead of the generic kernel; 0: never; 2: every pair it can take
 *   "wide_slots"        chunk slots per wave of the 512-thread geometry: 0 (default) = four on a batch's first align, three afterwards if that align showed they hold every pair; 3; 4
 *   "lane_max_len"      pairs whose longer sequence has at most this many bases try the one-wave-per-pair kernel first (default 325, weighed by the batch's divergence where it is known; 0: never)
 *   "mid_max_pairs"     a batch of at most this many pairs runs its mid-size pairs on the one-workgroup-per-pair kernel with every ring in LDS (default -1: one pair per CU; 0: never)
 *   "host_results"      1 (default): a score-only batch of up to 64 pairs gets its result arrays in pinned host memory (the mwf_gpu_batch_dev_*() pointers then point there); 0: device memory
 *   "div_aware"         1 (default): the size classes follow the batch's divergence (an 8-mer sketch of a few pairs: on the host while a batch is packed, on the device when one is wrapped); 0: lengths only
 *   "dev_retry"         1 (default): what the short-pair kernel hands back is re-run from a device-side list by a follow-up launch; 0: through the host
 *   "band_fold"         1 (default): score-only with o1 == x the packed kernel folds the gap-open row into its E1 / F1 registers (one row load less per chunk); 0: never
 *   "probe_table"       1 (default): the 512-thread packed kernel, default gap extensions, folded form, takes the first probe of its match extension from per-position 8-mer
 *                       tables in LDS (2 bytes per base of target + query) while two workgroups still share a CU; 0: never
 *   "band_fold2"        1 (default): score-only launches of that table form with e2 == 1, 3 <= o2 and o2 + e2 <= 16 also fold the row the second gap piece opens from into the
 *                       E2 / F2 registers one penalty ahead (two row loads per chunk instead of three; same s and n_iter); 0: never
 *   "alpha_remap"       0 (default): only pairs of plain A/C/G/T take the 2-bit copies.  1: on the first align of an uploaded batch, and on every align of a wrapped one, every pair
 *                       with at most four distinct bytes (mwf_alphabet_class 1: lower case, RNA, bases coded 0..3) is copied into a per-batch device arena with its bytes mapped onto A/C/G/T
 *                       and planned and aligned as a plain pair — same s, n_iter and CIGAR; summaries and maps keep reading the original bytes.  A wrapped batch's classes follow its current
 *                       contents (one small kernel and one wait per align) and pairs of five or more distinct bytes go straight to the byte-wise route.  The arena holds one copy of every such
 *                       pair (counted in dev_bytes, freed with the batch); if it does not fit what is free the batch runs as with 0.  The drop-in calls read MWF_ALPHA_REMAP=1 instead: the
 *                       variable is read once per process and applied to an engine when a call creates it, so it must be set before the first such call.  The batch's divergence estimate
 *                       ("div_aware") is still taken from the original bytes through (byte >> 1) & 3: lower case and U read as their upper-case letters, but codings that collapse under
 *                       it (bytes 0..3 read as 0, 0, 1, 1) can get other size classes, and so other re-run counts, than the plain twin — never other answers.
 *   "alpha16"           0 (default) or 1; acts only together with "alpha_remap" 1 (with "alpha_remap" 0: no buffer, no launch).  1: a pair of 5 to 16 distinct bytes (mwf_alphabet_class16
 *                       class 3: an N, IUPAC codes, soft-masked mixed case) is copied into the same arena with its bytes mapped to MWF_ALPHA16_TAG | code, whatever the penalties; every
 *                       kernel compares those image bytes as it would the originals — same s, n_iter and CIGAR.  Under gap extensions (2,1), with "seq2bit" / "band_pack" /
 *                       "band_span" not switched off, such a pair takes the packed band kernel's 4-bit form (mwf_band2_nib.hip: 512 threads x 3 or 4 chunk slots wherever a plain pair
 *                       would take a 64 ... 512-thread geometry, the span geometry where it would take the biased 512-thread copies or the span geometry) instead of the byte-wise
 *                       768-thread geometry or the generic kernel; the lane, mid, whole-device and generic routes and every other penalty set are as without it.  Pairs of 17 or more
 *                       distinct bytes (class 2) stay byte-wise.  MWF_ALPHA16=1 (read once per process) applies "alpha_remap" 1 and "alpha16" 1 to the engines the drop-in calls
 *                       create.  Not for batches of reads: those take the lane kernel's byte-wise copy either way and only pay for the copies.
 *   "trim"              (action) free the engine's workspace pools; they grow back on demand.
 * (The hooks tests and profiling scripts force kernels, geometries and failure paths with — "force_kind", "block", "sys_c" ... — are a separate, undeclared entry point,
 * mwf_gpu_test_hook in csrc/mwf_engine.cpp.) */
int mwf_gpu_set(mwf_gpu_t *g, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif

#endif
