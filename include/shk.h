/*
 * shk.h — C ABI of libshk, the MI355X-native k-mer counting engine.
 *
 * Drop-in boundary for the hot path of caseywdunn/sharkmer v3.1.0 (pure Rust,
 * no FFI seam of its own): the seam sits where the reference's src/io.rs calls
 * into src/kmer/ — drain_batch → Chunk::ingest_seq (io.rs:355-361,
 * kmer/chunk.rs:25-30) and consolidate_and_histogram →
 * KmerCounts::extend_with_histogram / Histogram::get_vector (io.rs:1021-1028).
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions (mirroring the reference's anyhow::Result-to-main behaviour,
 * SURVEY.md §8b): every function returns SHK_OK (0) or a negative SHK_ERR_*;
 * the message a reference run would have printed is available from
 * shk_last_error().  No exceptions, no unwinding, no torch types: plain
 * pointers and sizes only.  One caller thread per context (the reference's
 * counting is single-threaded); the library uses HIP streams internally.
 *
 * There is NO CPU fallback: shk_create fails with SHK_ERR_NO_DEVICE when no
 * gfx950 device is usable.
 */
#ifndef SHK_H
#define SHK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHK_ABI_VERSION 2

#define SHK_OK 0
#define SHK_ERR_INVALID_CHAR (-1) /* kmer/encoding.rs:353-356 */
#define SHK_ERR_BAD_ARG (-2)      /* cli.rs:659-677; encoding.rs:333 */
#define SHK_ERR_K_MISMATCH (-3)   /* counting.rs:158-160 */
#define SHK_ERR_NOMEM (-4)
#define SHK_ERR_NO_READS (-5)     /* io.rs:578-580 */
#define SHK_ERR_INVARIANT (-6)    /* io.rs:1042-1047, 1120-1132 */
#define SHK_ERR_FASTQ (-7)        /* io.rs:161-198, 287-318 */
#define SHK_ERR_IO (-8)
#define SHK_ERR_NO_DEVICE (-9)
#define SHK_ERR_HIP (-10)
#define SHK_ERR_STATE (-11)       /* call out of order / poisoned context */

#define SHK_READS_PER_BATCH 1000u /* N_READS_PER_BATCH, io.rs:15 */

/* flags */
#define SHK_FLAG_TIMING 1u        /* bracket every kernel with HIP events */
#define SHK_FLAG_FORCE_DIRECT 2u  /* count with the global-atomic kernel only */
#define SHK_FLAG_FORCE_PAGED 4u   /* count with the LDS-page kernels only */
#define SHK_FLAG_TIMING_SAMPLED 16u /* with SHK_FLAG_TIMING: only the launches of every 4th job are bracketed (a job =
                                    * what lies between two shk_reset calls; the first after shk_reset_timings is) — the
                                    * event records themselves cost ≈3 % of a 0.6 ms job */
#define SHK_RESERVE_NONE 0xFFFFFFFFu /* shk_config.reserve_cus: every compute unit, whatever SHK_RESERVE_CUS says */
#define SHK_FLAG_DEFER_ERRORS 8u  /* host-buffer ingests (shk_ingest_reads/_batch/_packed) return once their last
                                   * slice is queued, like the device-buffer ones: an invalid byte is reported by
                                   * the NEXT call on the context (ingest, sync, finalize), and that call's first
                                   * host-to-device copies overlap this one's counting */

#define SHK_FLAG_GROUP_GRAPH 32u   /* a multi-device context (n_devices > 1) answers sPCR's graph extension —
                                   * shk_neighborhood[_panel], shk_pcr_extend[_panel], shk_pcr_run — instead of refusing:
                                   * the search runs on the first device and each table probe reads the arrays of the
                                   * share that owns the key.  Opt-in because of what it has never been
                                   * run on: no run on more than one physical GPU has been possible where this was built,
                                   * and until this flag only copy engines (hipMemcpyPeerAsync) crossed devices.  With it a
                                   * kernel on one device dereferences another device's HBM.  On distinct cards two
                                   * things are written from the documentation and UNVERIFIED: whether the first device
                                   * sees the peers' latest table writes after the host-side stream synchronisations, and
                                   * what a dependent remote probe per level costs over xGMI.  Where peer access between
                                   * the first device and a distinct other one is missing the context is still created
                                   * and the graph calls answer SHK_ERR_STATE naming the two devices.  On a one-device
                                   * context the flag does nothing; owner shares (n_owners > 1) keep refusing. */
#define SHK_FLAG_GROUP_READS 64u   /* a multi-device context (n_devices > 1) retains reads and answers the retained calls —
                                   * shk_retain_reads, shk_retained_info, shk_retained_export, shk_filter_reads_panel_retained,
                                   * shk_thread_reads_panel_retained, and with SHK_FLAG_GROUP_GRAPH shk_pcr_run over
                                   * SHK_PCR_READS_RETAINED — instead of refusing: every device keeps the runs of reads the
                                   * exchange rounds deal it, walks its own store, and the host stitches the answers
                                   * (DESIGN.md §22).  No kernel reads another device's memory.  Opt-in: without it every
                                   * refusal stands.  On a one-device context and on owner shares the flag does nothing. */

typedef struct shk_ctx shk_ctx;

typedef struct shk_config {
  uint32_t k;          /* 0 < k < 32 (encoding.rs:333; CLI adds "odd", cli.rs:667) */
  uint32_t chunks;     /* CLI --chunks: 0 ⇒ one internal chunk and no histogram (io.rs:378) */
  uint64_t histo_max;  /* 0 < histo_max ≤ 1_000_000 (cli.rs:668-673) */
  int32_t device;      /* HIP device ordinal */
  uint32_t flags;      /* SHK_FLAG_* */
  uint64_t table_capacity_hint; /* expected distinct k-mers this context will hold; 0 = start small and grow.
                                   A multi-device context (n_devices > 1) splits it over its devices */
  /* OWNER SHARE ("alternative when local tables do not fit"): with n_owners = W > 1 (a
   * power of two ≤ 64) the context holds only the k-mers whose owner — the top log2(W) bits of the
   * engine's bijective key mix — is owner_id: 1/W of the key space, so W contexts (one per GPU) together
   * hold every k-mer exactly once and no table is ever exchanged.  shk_ingest_* on such a context counts
   * the owned k-mers of the reads it is given and drops the rest; the shk_xchg_* entry points below
   * partition a batch's records by owner for an exchange between the W contexts instead.  Read/base
   * counters count every read handed over; k-mer counters and histograms cover the owned share
   * (histogram bins are additive across shares: KmerCounts::extend over disjoint key sets,
   * counting.rs:157-166, io.rs:1023-1028).  "Handed over" is the share's own view: n_reads_ingested, n_bases_read and
   * n_bases_ingested count the batches given to shk_ingest_* on THIS context and the batches THIS context scattered
   * (shk_xchg_scatter_device, _begin, shk_xchg_wide_scatter_device), whether or not anybody absorbed the round's
   * segments afterwards; shk_xchg_absorb and shk_insert_device add nothing to them.  Over the shares of an exchange
   * job they add up to the job's reads (every read is scattered once), in drop mode to W times that; a round that was
   * scattered and given up stays in the scattering share's counters until its shk_reset.  shk_finalize on a share that
   * was handed nothing does not fail with SHK_ERR_NO_READS: the caller looks at the sum over the shares.
   * 0: the whole key space.  1: the whole key space AS A SHARE — the
   * context takes the shk_xchg_* rounds like any owner share (one segment), so that the exchange path of a
   * W-process job runs unchanged in a world of one. */
  uint32_t n_owners;
  uint32_t owner_id;
  /* MULTI-DEVICE CONTEXT (SURVEY.md §8b `n_devices, device_ids`): n_devices > 1 makes ONE context that
   * spans device_ids[0..n_devices) (a power of two ≤ 64 devices; an id may repeat — the test rigs put
   * several shares on one card): one owner share per device, host batches of 1000 reads dealt round-robin
   * to the devices with their global read index (io.rs:340-361), records exchanged by owner between the
   * devices during ingest, one histogram sum at finalize.  `device` is ignored then.  0 or 1: one device. */
  uint32_t n_devices;
  /* COMPUTE UNITS LEFT FREE (round 4): the context's PERSISTENT kernel — the 4-byte-record scatter, one 1024-thread
   * workgroup with 144 of 160 KiB of LDS on every CU for the whole launch — starts this many workgroups fewer (rounded
   * up to a multiple of 8), so that whoever else works on the card while it counts finds a CU: the collectives of a
   * multi-GPU job, whose channels are workgroups that need CUs and LDS while a round's segments travel under the next
   * round's scatter.  (The other kernels are many short workgroups; a collective's get in as those retire.)
   * 0: the default — none for a whole-key-space context, SHK_RESERVE_CUS (default 16) for an owner share of a
   * multi-GPU job (n_owners > 1); SHK_RESERVE_NONE (~0): none, whatever the environment says.  What it costs the
   * counting on one card is in DESIGN.md §6. */
  uint32_t reserve_cus;
  const int32_t *device_ids;
  uint64_t reserved[1];
} shk_config;

/* io.rs:545-552 and counting.rs:254-260 totals, plus device-side facts */
typedef struct shk_counters {
  uint64_t n_reads_ingested;  /* Σ Chunk::n_reads (chunk.rs:27) */
  uint64_t n_bases_read;      /* Σ sequence lengths, N included (io.rs:335) */
  uint64_t n_bases_ingested;  /* Σ Chunk::n_bases = non-N bytes (chunk.rs:28) */
  uint64_t n_kmers_ingested;  /* Σ over chunks of Σ table counts (io.rs:550) */
  uint64_t n_unique_kmers;    /* merged table len (counting.rs:258) — valid after finalize */
  uint64_t n_hashed_kmers;    /* Σ merged counts (io.rs:1035) — valid after finalize */
  uint64_t n_singleton_kmers; /* last column [1] (io.rs:1096-1099) — chunks>0 only */
  uint32_t any_saturated;     /* counting.rs:190-200 */
  uint32_t n_chunks;          /* internal chunk count (≥1) */
  uint64_t table_capacity;    /* slots */
  uint64_t n_grows;           /* table doublings so far */
  uint64_t n_spilled;         /* k-mers that took the spill path */
} shk_counters;

/* Accumulated per-kernel device time (HIP events on the engine's stream);
 * filled only when SHK_FLAG_TIMING is set. */
#define SHK_N_KERNELS 16
typedef struct shk_timings {
  double ms[SHK_N_KERNELS];
  uint64_t launches[SHK_N_KERNELS];
} shk_timings;
/* kernel ids for shk_timings */
enum {
  SHK_K_MARK = 0,      /* read-start bitmap + tile list */
  SHK_K_SCAN = 1,      /* validate / count bases / partition histogram */
  SHK_K_DIRECT = 2,    /* extract + global-atomic insert */
  SHK_K_SCATTER = 3,   /* extract + LDS-sorted partition scatter (k_part_scatter_sorted) */
  SHK_K_PAGES = 4,     /* LDS page count */
  SHK_K_HISTO = 5,     /* table scan → histograms + totals */
  SHK_K_GROW = 6,      /* rehash into a bigger table */
  SHK_K_INSERT = 7,    /* (kmer,count) insert / spill re-insert */
  SHK_K_LOOKUP = 8,
  SHK_K_EXPORT = 9,
  SHK_K_SYNTH = 10,
  SHK_K_MERGE = 11,
  SHK_K_PCOUNT = 12,   /* validate + count k-mers per partition (k_part_count) */
  SHK_K_PSCAN = 13,    /* the two small exclusive scans between count and scatter */
  SHK_K_HISTO_ROWS = 14, /* histograms + totals from the rows the (one) fresh page pass of a job left behind, instead of SHK_K_HISTO's scan */
  SHK_K_EXTEND = 15    /* shk_neighborhood(_panel): seed, narrow and wide level launches, a panel's pack */
};

/* ---- lifecycle ------------------------------------------------------------ */

/* Replaces Chunk::new ×n_chunks (io.rs:378-379) + Histogram::new (io.rs:1021).
 * Validates the cli.rs:659-677 ranges except "k odd" (a CLI rule; the kmer
 * module itself accepts any 0<k<32, encoding.rs:333). */
int shk_create(const shk_config *cfg, shk_ctx **out);
/* Drop of FastqReadState / KmerCounts. */
void shk_destroy(shk_ctx *ctx);
/* Back to the state right after shk_create (empty chunks, zero counters), keeping the
 * allocated table and scratch: a fresh FastqReadState (io.rs:381-387) without re-allocating. */
int shk_reset(shk_ctx *ctx);
/* The anyhow message of the last failure on this context ("" if none).
 * ctx == NULL returns the message of the last failed shk_create on this thread. */
const char *shk_last_error(const shk_ctx *ctx);
int shk_abi_version(void);

/* ---- ingest ----------------------------------------------------------------- */

/* Replaces the body of drain_batch (io.rs:356-358): every sequence of the
 * batch goes to chunk `chunk_id` (Chunk::ingest_seq, chunk.rs:25-30).
 * bases: concatenated ASCII sequences; offsets[n_seqs+1] byte offsets into
 * bases.  Host buffers, caller-owned, may be freed after return.
 * Any byte outside ACGTN ⇒ SHK_ERR_INVALID_CHAR, message identical to
 * encoding.rs:353-356, context poisoned (the reference aborts the run). */
int shk_ingest_batch(shk_ctx *ctx, uint32_t chunk_id, const uint8_t *bases,
                     const uint64_t *offsets, uint64_t n_seqs);

/* Replaces read_fastq's push + drain_batch cadence (io.rs:335-343, 355-361)
 * for a run of sequences in input order: the engine keeps the running read
 * index i and sends read i to chunk (i / 1000) % n_chunks. */
int shk_ingest_reads(shk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets,
                     uint64_t n_seqs);

/* ---- 2-bit packed input ---------------------------------------------------------------------------------
 * The layout of the reference's Read::from_str (src/kmer/encoding.rs:60-95; known-answer vectors
 * src/kmer/mod.rs:61-156) applied to a batch's concatenated bases as ONE sequence: 4 bases per byte, the first
 * base in the two most significant bits (A 00, C 01, G 10, T 11), the tail left-aligned in its byte; plus an
 * N mask — bit p % 32 of word p / 32 set where base p is N (code 00 in the stream) — because
 * kmers_from_ascii, unlike from_str, takes N (encoding.rs:346-352).  0.28 B/base instead of 1 over PCIe.
 * shk_pack_reads (host, n_threads = 0: all cores) validates like encoding.rs:353-356: the first byte outside
 * ACGTN in input order ⇒ SHK_ERR_INVALID_CHAR, message from shk_run_error().  packed: (n_bases+3)/4 bytes,
 * nmask: (n_bases+31)/32 words (shk_packed_sizes). */
void shk_packed_sizes(uint64_t n_bases, uint64_t *packed_bytes, uint64_t *nmask_words);
int shk_pack_reads(const uint8_t *bases, uint64_t n_bases, uint8_t *packed, uint32_t *nmask, uint32_t n_threads);
/* shk_ingest_reads for a packed batch: offsets[n_seqs+1] are BASE indices into the stream (offsets[0] is
 * where the batch starts in it).  Host buffers. */
int shk_ingest_packed(shk_ctx *ctx, const uint8_t *packed, const uint32_t *nmask, const uint64_t *offsets,
                      uint64_t n_seqs);
/* The same with everything resident in device memory (the stream starts at base 0; d_offsets as in
 * shk_ingest_reads_device).  Asynchronous like shk_ingest_reads_device. */
int shk_ingest_packed_device(shk_ctx *ctx, const void *d_packed, const void *d_nmask, const void *d_offsets,
                             uint64_t n_seqs, uint64_t n_bases);
/* The packer and its inverse on the device (ASCII bytes ↔ stream + mask, all device pointers): what the
 * device-side buffer of a batch looks like, pinned by the reference's vectors in tests/test_gpu_packed.py.
 * shk_pack_reads_device reports an invalid byte like shk_pack_reads (message from shk_last_error) and leaves
 * the context usable. */
int shk_pack_reads_device(shk_ctx *ctx, const void *d_bases, uint64_t n_bases, void *d_packed, void *d_nmask);
int shk_unpack_reads_device(shk_ctx *ctx, const void *d_packed, const void *d_nmask, uint64_t n_bases, void *d_bases);

/* Set the running read index used by shk_ingest_reads* for chunk striping (default 0).  A
 * host that shards one input stream over several contexts/GPUs gives each shard the global
 * index of its first read, so that read i still lands in chunk (i / 1000) % n_chunks. */
int shk_set_read_index(shk_ctx *ctx, uint64_t next_read_index);

/* Same as shk_ingest_reads with input already resident in device memory
 * (d_bases: n_bases bytes, d_offsets: n_seqs+1 u64).  Asynchronous on the
 * engine stream; errors surface at the next synchronising call. */
int shk_ingest_reads_device(shk_ctx *ctx, const void *d_bases, const void *d_offsets,
                            uint64_t n_seqs, uint64_t n_bases);

/* Replaces KmerCounts::insert (counting.rs:152-154) on chunk `chunk_id`:
 * saturating add of counts[i] to kmers[i]. Host buffers. */
int shk_insert_counts(shk_ctx *ctx, uint32_t chunk_id, const uint64_t *kmers,
                      const uint32_t *counts, uint64_t n);

/* Wait for all queued device work; report deferred errors. */
int shk_sync(shk_ctx *ctx);

/* ---- consolidate ----------------------------------------------------------- */

/* Replaces the merge loop of consolidate_and_histogram (io.rs:1023-1028 for
 * chunks>0, io.rs:1135-1138 for chunks==0) and its invariants
 * (io.rs:1042-1047, 1120-1132).  SHK_ERR_NO_READS mirrors io.rs:578-580.
 * Idempotent; ingest after finalize re-opens the context. */
int shk_finalize(shk_ctx *ctx);
/* shk_finalize in two halves — histo_vecs (io.rs:1020-1028) of the UNION of several contexts' reads, bins being
 * additive over disjoint key sets (KmerCounts::extend, counting.rs:157-166) — for a caller that sums histograms
 * over several contexts ON THE DEVICE (one process
 * per GPU: an in-place all-reduce of *d_sum over the ranks, queued on shk_stream(), instead of a host round trip
 * through shk_histograms).  _begin queues the scan and hands out the block a reduction may SUM — n_words u64:
 * the totals, the per-lane base counts, four bookkeeping words (reads ingested, bases read, "my scan ran over a
 * table that still had to be repaired", user_word), the histogram.  _end brings the block back (one host sync for
 * everything queued so far) and repairs this context's table if its last launch had spilled records; *again = 1
 * when ANY context's had — the same sum on every rank — in which case nothing is final and every rank repeats
 * _begin / reduction / _end.  Afterwards shk_histograms and shk_get_counters (n_reads_ingested, n_bases_*,
 * n_kmers_ingested, n_unique_kmers, n_hashed_kmers) report what the reduction left: the whole job's.  The
 * io.rs:1042-1047 invariants are the caller's to check on the summed numbers.  *user_sum: Σ user_word. */
int shk_finalize_begin(shk_ctx *ctx, uint64_t user_word, void **d_sum, uint64_t *n_words);
int shk_finalize_end(shk_ctx *ctx, int *again, uint64_t *user_sum);

/* histo_vecs of io.rs:1020-1028: chunks × (histo_max+2) u64, row-major by
 * chunk; column j = Histogram::get_vector() after merging chunks 0..j
 * (histogram.rs:125-134).  chunks==0 ⇒ nothing is written, returns SHK_OK. */
int shk_histograms(shk_ctx *ctx, uint64_t *out);

int shk_get_counters(shk_ctx *ctx, shk_counters *out);
int shk_get_timings(shk_ctx *ctx, shk_timings *out);
int shk_reset_timings(shk_ctx *ctx);
/* The materialising page pass of a context whose last counting launch left its table unwritten (a histogram job's
 * fresh fused page pass writes no table; the first reader or writer of the table has it written then): device time and
 * timed launches since shk_reset_timings, under SHK_FLAG_TIMING like the slots of shk_timings — whose layout is fixed
 * by this ABI version, hence a call of its own.  Either pointer may be null. */
int shk_get_lazy_table_timing(shk_ctx *ctx, double *ms, uint64_t *launches);
/* Cursor segments per page region of the context's last paged counting launch (0: there has been none; a group: its
 * first device's): 1 everywhere but where k_scatter32 writes straight into the regions k_pages32 reads. */
int shk_get_scatter_segments(shk_ctx *ctx, uint32_t *segs);

/* ---- merged-table read API (counting.rs:205-260) --------------------------------- */

/* KmerCounts::iter (counting.rs:239-241) over the merged table: writes up to
 * cap (kmer,count) pairs in unspecified order; *n_out = number of entries. */
int shk_export_table(shk_ctx *ctx, uint64_t *kmers, uint32_t *counts, uint64_t cap,
                     uint64_t *n_out);
/* KmerCounts::get_count (canonical=0, counting.rs:224-226) or
 * get_canonical_count (canonical=1: min(kmer, revcomp), counting.rs:205-209). */
int shk_lookup(shk_ctx *ctx, const uint64_t *kmers, uint32_t *counts, uint64_t n,
               int canonical);

/* find_oligos_in_kmers (src/pcr/primers.rs:163-226), sPCR's primer seed scan over the merged
 * table: oligos[] are 2-bit encoded values of oligo_len bases (1 ≤ oligo_len < k).  A k-mer
 * with merged count ≥ min_count whose FIRST oligo_len bases equal an oligo is reported as is;
 * one whose LAST oligo_len bases equal an oligo's reverse complement is reported
 * reverse-complemented (primers.rs:212-223).  Same output convention as shk_export_table. */
int shk_find_oligos(shk_ctx *ctx, const uint64_t *oligos, uint32_t n_oligos, uint32_t oligo_len,
                    uint32_t min_count, uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n_out);

/* One primer direction of sPCR's seed discovery: PCRParams' forward_seq or reverse_seq with the fields
 * get_primer_kmers reads (src/pcr/primers.rs:234-480; defaults of pcr/mod.rs's PCRParams in brackets). */
typedef struct shk_primer {
  const char *seq;     /* IUPAC primer as written (ACGTRYWSKMBDHVN, upper case) */
  uint32_t trim;       /* [15] keep the last trim bases; trim ≥ k is clamped to k−1 (primers.rs:244-271) */
  uint32_t mismatches; /* [2] mismatch levels 0..=min(mismatches, trimmed length) (primers.rs:286-313) */
  uint32_t min_count;  /* [2] a table k-mer counts when its merged count ≥ min_count (primers.rs:212) */
  uint32_t max_kmers;  /* [40] max_primer_kmers: the cap filled level by level (primers.rs:375-438) */
} shk_primer;

#define SHK_PRIMER_LEVELS 33 /* level slots per primer in n_variants / level_hits (levels ≤ k−1 ≤ 30) */

/* preprocess_primer_by_mismatch (primers.rs:237-313) for a table of k-mers of length k, on the host (no device
 * touched, no context needed): *trimmed_len = L, the length of the trimmed primer P; *n_levels = min(mismatches, L) + 1
 * (0 when P is empty: trim 0 or an empty primer — then nothing is searched and nothing fails);
 * n_variants[m] = |level m| for m < *n_levels, 0 above (the variant sets are never listed).
 * Errors (text in err, at most err_len bytes with the terminating NUL; "" on success):
 *   SHK_ERR_BAD_ARG      more than 10000 resolved variants, the reference's text (primers.rs:273-284);
 *   SHK_ERR_INVALID_CHAR a character of P outside the IUPAC codes, "Invalid nucleotide {c} in {variant}"
 *                        (string_to_oligo, primers.rs:33-55) — only when max_kmers > 0 and P is not empty, as the
 *                        reference converts a variant only in a non-empty round it runs (primers.rs:383-393). */
int shk_primer_compile(const shk_primer *p, uint32_t k, uint32_t *trimmed_len, uint32_t *n_levels,
                       uint64_t *n_variants, char *err, size_t err_len);

/* get_primer_kmers (primers.rs:234-480) for n_primers primer directions in ONE pass over the merged table (the
 * owned pages of an owner share; every share of a multi-device context, then selected over their union).  A table
 * k-mer x with merged count c ≥ min_count, whose first L bases have f mismatches against P and whose reverse
 * complement's first L bases have r, yields (x, c) at level f when f ≤ M, and (revcomp(x), c) at level r when
 * r ≤ M and r ≠ f (the `else if` of find_oligos_in_kmers, primers.rs:212-223, within one level's pass).
 * Primer i's result is kmers/counts/levels[offsets[i] .. offsets[i+1]) (offsets: n_primers + 1 entries), the first
 * max_kmers hits in the order level ascending, count descending, k-mer ascending — the insertion order of
 * discover_primer_kmers_by_round (primers.rs:375-438).  level_hits (optional, n_primers × SHK_PRIMER_LEVELS):
 * hits at level m before the cap (the reference's "Mismatch level m: n new primer kmers … dropped d" is n + d);
 * all zero for a primer with max_kmers = 0 or an empty P, which is not searched.  cap ≥ Σ max_kmers.
 * Errors: the too-many-variants check of every primer first (in order), then the invalid-character check of every
 * searched one — for a forward/reverse pair that is the reference's order (primers.rs:440-478).  The selection
 * does not merge equal output k-mers: the table holds canonical k-mers, so two entries never yield the same one.
 * Tuning: SHK_PRIMER_CANDIDATES (records, read at each call) bounds the first pass's candidate buffer; when it
 * overflows, each primer's level counts give its cut level and the pass is rerun keeping only levels up to it. */
int shk_primer_kmers(shk_ctx *ctx, const shk_primer *primers, uint32_t n_primers, uint64_t *kmers,
                     uint32_t *counts, uint8_t *levels, uint64_t cap, uint64_t *offsets, uint64_t *level_hits);

/* PrimerReadFilter::matches over a batch (src/pcr/read_filter.rs:24-55), the read selection in front
 * of sPCR's read threading: out_matches[i] = 1 when read i has no byte outside ACGTN (otherwise
 * kmers_from_ascii fails and the reference returns false for the read) and at least one of its
 * canonical k-mers (k of the context) is among primer_kmers[] (canonical 2-bit k-mers, the union
 * of the forward and reverse primer tables), else 0.  Host buffers; the context's table is not
 * touched. */
int shk_filter_reads(shk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                     const uint64_t *primer_kmers, uint64_t n_kmers, uint8_t *out_matches);

/* Batched kmers_from_ascii (src/kmer/encoding.rs:332-371) as sPCR's read threading calls it
 * (src/pcr/threading.rs:97-101, also pcr/read_filter.rs:44): read i's canonical k-mers, in read
 * order, are kmers[koff(i) .. koff(i) + n_kmers[i]) with koff(i) = Σ_{r<i} max(0, len_r − k + 1),
 * the most a read can yield (an N shortens it: n_kmers[i] ≤ max(0, len_i − k + 1); the rest of the
 * read's span is left untouched).  bad_byte[i] = 0, or the first byte outside ACGTN: such a read
 * is the reference's Err (message of encoding.rs:353-356 with that byte) and yields no k-mers
 * (n_kmers[i] = 0), which is how thread_reads treats it (threading.rs:99-101: skipped).
 * kmers_cap must be ≥ koff(n_seqs).  Host buffers; the context's table is not touched. */
int shk_kmers_from_reads(shk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                         uint64_t *kmers, uint64_t kmers_cap, uint32_t *n_kmers, uint8_t *bad_byte);

/* threading::thread_reads / thread_reads_paired (src/pcr/threading.rs:87-192, called at src/pcr/mod.rs:663-697): a
 * batch of reads threaded through a graph on the device; what comes back is the annotation, not the k-mers.
 * GRAPH: any graph as arrays — node v = position v of node_sub_kmers (a (k−1)-mer ≤ (1 << 2(k−1)) − 1, k of the
 *   context), edge e = position e of edge_src / edge_tgt (node positions): the surviving nodes and edges of the caller's
 *   StableDiGraph in ascending NodeIndex / EdgeIndex, which is the form shk_pcr_extend hands out.
 * EDGE K-MER: (sub_kmer[src] << 2) | (sub_kmer[tgt] & 3) (reconstruct_edge_kmer, graph.rs:127-134), whether or not the
 *   two nodes overlap; its lookup key is min(x, revcomp(x)).  The CANDIDATES of a key are all edges with that key in
 *   ascending edge index (build_edge_lookup, threading.rs:203-220) — any number of them, as the reference's SmallVec.
 * PER READ: the list of kmers_from_ascii (encoding.rs:332-371): an N drops the windows that contain it and leaves no
 *   gap, so the k-mers either side of it are neighbours in the list.  A byte outside ACGTN anywhere in the read makes
 *   the read contribute nothing (threading.rs:98-101; read_edges = 0) and is no error of the call.  Walking the list
 *   (find_contiguous_runs + resolve_candidates, threading.rs:233-315): prev = the edge chosen for the previous element
 *   if that element had candidates, else none; an element with candidates chooses the first whose source is
 *   tgt(prev), or candidate 0 when there is none or no prev; a run breaks before an element when the previous one had
 *   no candidates or tgt(prev) != src(chosen); an element without candidates is in no run.
 * PER RUN (threading.rs:106-118, 321-364): degrees are edge counts (parallel edges count severally, a self-loop in
 *   both), v is a BRANCH NODE when in_deg(v) > 1 or out_deg(v) > 1.  Every consecutive pair (a, b) of a run whose
 *   v = tgt(a) is a branch node adds 1 to the link (a, b) and makes the run ambiguous.  Every element of a run adds 1
 *   to support_total of its edge (per occurrence), and in an unambiguous run to support_unambiguous too; a run of
 *   one element is unambiguous.
 * PAIRED (read_index and mate both given; mate 0 unpaired, 1 R1, 2 R2): the same annotations, and n_paired_links =
 *   the distinct read_index / 2 for which some R1 read and some R2 read each mapped to at least one edge
 *   (threading.rs:166-189); both mates of a pair have to be in one call.
 * OUT: per call (additive over batches, n_paired_links excepted).  Links ascending by (in, out); link_cap too small:
 *   SHK_ERR_BAD_ARG with n_links set to the need (the other outputs are complete then).  n_edges == 0 or n_seqs == 0:
 *   all zero.
 * Errors, SHK_ERR_BAD_ARG: an endpoint ≥ n_nodes, a sub_kmer above the mask, k < 2, n_nodes or n_edges ≥ 2^32,
 *   decreasing offsets, one of read_index / mate without the other, mate > 2; also a read of 2^31 bases or more, and a
 *   graph whose branch nodes have more than 2^31 (incoming, outgoing) pairs between them — every such pair has a
 *   counter of its own on the device.
 * The context's table is neither read nor written; valid whenever shk_filter_reads is, on owner shares too; a
 * multi-device context runs it on its first device.  The call is shk_thread_reads_panel (below) for one gene that lists
 * every read of the batch in the batch's order — the same launch, with no list uploaded.  Tuning, all read at each
 * call, none changes the result: SHK_THREAD_LDS_EDGES (edges; default 2048): graphs up to that size keep their lookup
 * set in LDS, larger ones in global memory; SHK_THREAD_PANEL_JOB and SHK_THREAD_PANEL_BLOCKS cut this call's batch and
 * cap its workgroups as they do a panel's.  With SHK_TRACE set the launch prints the panel's line (1 genes). */
typedef struct shk_thread_out {   /* every pointer optional except the two support arrays */
  uint32_t *support_total;        /* [n_edges] EdgeReadSupport.read_support_total        */
  uint32_t *support_unambiguous;  /* [n_edges] EdgeReadSupport.read_support_unambiguous  */
  uint32_t *link_in, *link_out, *link_counts; uint64_t link_cap, n_links;  /* BranchLink -> count */
  uint32_t *read_edges;           /* [n_seqs] edges this read was mapped to (sum of its run lengths) */
  uint64_t n_paired_links;        /* thread_reads_paired's paired_links.len(); 0 when mate == NULL */
} shk_thread_out;
/* Host buffers (bases / offsets as shk_ingest_reads): stages the batch, then as the device form. */
int shk_thread_reads(shk_ctx *ctx, const uint64_t *node_sub_kmers, uint64_t n_nodes,
                     const uint32_t *edge_src, const uint32_t *edge_tgt, uint64_t n_edges,
                     const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                     const uint64_t *read_index, const uint8_t *mate, /* both NULL: thread_reads; else thread_reads_paired */
                     shk_thread_out *out);
/* The batch resident in device memory (d_bases: n_bases bytes, d_offsets: n_seqs + 1 u64, as shk_ingest_reads_device);
 * everything else on the host.  Returns when the annotation is complete. */
int shk_thread_reads_device(shk_ctx *ctx, const uint64_t *node_sub_kmers, uint64_t n_nodes,
                            const uint32_t *edge_src, const uint32_t *edge_tgt, uint64_t n_edges,
                            const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                            const uint64_t *read_index, const uint8_t *mate, shk_thread_out *out);

/* shk_thread_reads for a whole sPCR panel in ONE call: do_pcr threads each gene's filtered reads through that gene's
 * pruned graph (src/pcr/mod.rs:663-697, src/pcr/threading.rs:87-192); this call takes every graph of the panel, the
 * per-gene read lists as shk_filter_reads_panel returns them and the batch where it lies, and answers for all genes
 * from one launch — no gather, no second copy of the reads.
 * GRAPHS: gene g's graph is nodes node_sub_kmers[node_offsets[g] .. node_offsets[g+1]) and edges
 *   [edge_offsets[g] .. edge_offsets[g+1]) of edge_src / edge_tgt, whose entries are node positions LOCAL to the gene
 *   (0 = the gene's first node): the output of shk_pcr_extend_panel as it is, n_genes outputs of shk_pcr_extend, or the
 *   caller's pruned graphs, concatenated without renumbering.  Each graph follows the rules of shk_thread_reads: EDGE
 *   K-MER, candidates ascending by edge (build_edge_lookup, threading.rs:203-220), degrees as edge counts
 *   (threading.rs:329-330).  All three offset arrays have n_genes + 1 entries, non-decreasing.
 * LISTS: gene g's reads are list_reads[list_offsets[g] .. list_offsets[g+1]), indices into the batch — exactly the
 *   match_offsets / match_reads of shk_filter_reads_panel.  Any order is accepted, a read may be in any number of
 *   genes, and a repeat inside a list counts twice, as it would in a gathered batch.
 * RESULT: for every g, what shk_thread_reads gives for gene g's graph over the batch made of its listed reads in list
 *   order (threading.rs:87-192): support_* at edge_offsets[g] .., the links ascending by (in, out) at
 *   [link_offsets[g], link_offsets[g+1]) with edge indices LOCAL to the gene, read_edges per list position.  With
 *   read_index and mate given (indexed by read of the BATCH, n_seqs entries each), n_paired_links[g] = the distinct
 *   read_index / 2 for which some listed R1 read and some listed R2 read of gene g each mapped to an edge
 *   (threading.rs:166-189).
 * DEGENERATE: a gene with no edges: its read_edges are 0; a gene with no reads: its supports are 0; n_genes == 0:
 *   all zero; a read with a byte outside ACGTN contributes nothing and is no error (threading.rs:98-101).
 * link_cap too small: SHK_ERR_BAD_ARG with n_links set to the need and link_offsets complete; the other outputs are
 *   complete too, as in shk_thread_reads.
 * Errors, SHK_ERR_BAD_ARG with a text that names the gene, all raised before the device is touched (the device form
 *   has to copy the read offsets back to check them): every graph error of shk_thread_reads; decreasing node_offsets,
 *   edge_offsets, list_offsets or read offsets; a listed read ≥ n_seqs; n_genes > SHK_THREAD_MAX_GENES; one of
 *   read_index / mate without the other; mate > 2; a panel with 2^32 edges or more in total; a panel with more than
 *   2^31 link slots ((incoming, outgoing) pairs at branch nodes) in total.
 * The context's table is neither read nor written; valid whenever shk_thread_reads is, on owner shares too; a
 * multi-device context runs it on its first device.  Tuning, all read at each call, none changes the result:
 * SHK_THREAD_LDS_EDGES decides per gene, as for shk_thread_reads, whether the gene's set goes to LDS;
 * SHK_THREAD_PANEL_JOB (reads, default 16): every list is cut into slices of at most that many reads, the jobs the
 * workgroups share out; SHK_THREAD_PANEL_BLOCKS (0 = a wave per listed read up to the device's workgroups) caps the
 * workgroups.  Both hold for shk_thread_reads[_device] too, which is this call with one gene. */
#define SHK_THREAD_MAX_GENES 4096   /* = SHK_FILTER_MAX_GENES: the lists come from that call */
typedef struct shk_thread_panel_out {  /* every pointer optional except the two support arrays */
  uint32_t *support_total;        /* [edge_offsets[n_genes]] gene g's edges at edge_offsets[g] ..            */
  uint32_t *support_unambiguous;  /* same layout                                                           */
  uint64_t *link_offsets;         /* [n_genes + 1] gene g's links are [link_offsets[g], link_offsets[g+1])   */
  uint32_t *link_in, *link_out, *link_counts; uint64_t link_cap, n_links;  /* edge indices LOCAL to the gene */
  uint32_t *read_edges;           /* [list_offsets[n_genes]] aligned with list_reads                         */
  uint64_t *n_paired_links;       /* [n_genes]; zeros when mate == NULL                                      */
} shk_thread_panel_out;
/* Host buffers (bases / offsets as shk_ingest_reads): stages the batch, then as the device form. */
int shk_thread_reads_panel(shk_ctx *ctx, const uint64_t *node_sub_kmers, const uint64_t *node_offsets,
                           const uint32_t *edge_src, const uint32_t *edge_tgt, const uint64_t *edge_offsets, uint32_t n_genes,
                           const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                           const uint64_t *list_offsets, const uint64_t *list_reads,
                           const uint64_t *read_index, const uint8_t *mate, shk_thread_panel_out *out);
/* The batch resident in device memory (d_bases: n_bases bytes, d_offsets: n_seqs + 1 u64, as shk_ingest_reads_device);
 * everything else on the host.  The offsets are copied back once.  Returns when the annotations are complete. */
int shk_thread_reads_panel_device(shk_ctx *ctx, const uint64_t *node_sub_kmers, const uint64_t *node_offsets,
                                  const uint32_t *edge_src, const uint32_t *edge_tgt, const uint64_t *edge_offsets, uint32_t n_genes,
                                  const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                                  const uint64_t *list_offsets, const uint64_t *list_reads,
                                  const uint64_t *read_index, const uint8_t *mate, shk_thread_panel_out *out);

/* PrimerReadFilter::filter_reads (src/pcr/read_filter.rs:24-55) for a whole sPCR panel in ONE pass over the batch:
 * do_pcr runs once per gene (stats.rs:85-87) and filters every retained read against that gene's primer k-mers
 * (pcr/mod.rs:470-485); this call walks the reads once and answers for all n_genes genes.
 * PANEL: gene g's primer set is primer_kmers[gene_offsets[g] .. gene_offsets[g+1]) (gene_offsets: n_genes + 1 entries,
 *   non-decreasing): canonical 2-bit k-mers (k of the context), the union of the gene's forward and reverse tables
 *   (from_primer_kmers, read_filter.rs:24-41).  Duplicates inside a gene are allowed, a k-mer may be in any number
 *   of genes, a gene may be empty.  n_genes ≤ SHK_FILTER_MAX_GENES: every wave of the kernel keeps one bit per gene in
 *   LDS, 512 bytes × the 16 waves of a workgroup at the limit.
 * MATCH: read i matches gene g exactly when PrimerReadFilter::matches (read_filter.rs:43-49) is true for it against
 *   g's set: no byte outside ACGTN anywhere in the read, and at least one of its kmers_from_ascii k-mers in the set.
 *   A window that contains an N is not a k-mer; a read shorter than k matches nothing; a read with an invalid byte,
 *   wherever it lies, matches no gene and is no error of the call.
 * OUT: match_reads[match_offsets[g] .. match_offsets[g+1]) are the indices of the reads that match gene g, ascending —
 *   the order of filter_reads (read_filter.rs:52-54); match_offsets has n_genes + 1 entries, *n_matches is the total.
 *   match_cap too small: SHK_ERR_BAD_ARG with *n_matches set to the need and match_offsets complete.  n_genes == 0 or
 *   n_seqs == 0: all zero.  With n_genes == 1 the list is the positions where shk_filter_reads writes 1.
 * Errors, SHK_ERR_BAD_ARG: decreasing gene_offsets or read offsets, a k-mer that does not fit k bases, a read of 2^31
 *   bases or more, n_genes above SHK_FILTER_MAX_GENES.
 * The context's table is neither read nor written; valid whenever shk_filter_reads is, on owner shares too; a
 * multi-device context runs it on its first device.  Tuning, both read at each call, neither changes the result:
 * SHK_FILTER_LDS_KEYS (distinct k-mers of the panel, default 4096): panels up to that size keep their lookup set in
 * LDS (if it fits 128 KiB), larger ones in global memory; SHK_FILTER_CANDIDATES ((gene, read) records, default 2^20)
 * sizes the first pass's record list — when it overflows, the pass has counted the records and is rerun with room
 * for exactly that many. */
#define SHK_FILTER_MAX_GENES 4096
/* Host buffers (bases / offsets as shk_ingest_reads): stages the batch, then as the device form. */
int shk_filter_reads_panel(shk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                           const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes,
                           uint64_t *match_offsets, uint64_t *match_reads, uint64_t match_cap, uint64_t *n_matches);
/* The batch resident in device memory (d_bases: n_bases bytes, d_offsets: n_seqs + 1 u64, as shk_ingest_reads_device);
 * the panel and the outputs on the host. */
int shk_filter_reads_panel_device(shk_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                                  const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes,
                                  uint64_t *match_offsets, uint64_t *match_reads, uint64_t match_cap, uint64_t *n_matches);
/* A subset of a device-resident batch as a batch of its own, on the device — what carries a gene's match list to
 * shk_thread_reads_device without the reads leaving HBM.  read_ids (host; any order, repeats allowed, each below
 * n_seqs) name reads of (d_bases, d_offsets); they are copied into d_out_bases back to back in list order,
 * d_out_offsets gets n_ids + 1 u64 starting at 0, *n_out_bases is the total.  The call copies d_offsets back (8 bytes
 * per read) to size and place the output.  out_bases_cap too small: SHK_ERR_BAD_ARG with *n_out_bases set to the need
 * and nothing written.  Also SHK_ERR_BAD_ARG: an id ≥ n_seqs, decreasing offsets.  Stateless like the filter. */
int shk_gather_reads_device(shk_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs,
                            const uint64_t *read_ids, uint64_t n_ids,
                            void *d_out_bases, uint64_t out_bases_cap, void *d_out_offsets, uint64_t *n_out_bases);

/* RETAINED READS: the reads of a job kept in device memory as they are ingested, so that sPCR's read pass (the two
 * _retained calls below) needs no second pass over the input — the reference re-opens its files and collects every
 * sequence on the host (reread_sequences, src/io.rs:769-943, from src/main.rs:134).  The store holds three bit planes
 * (code bit 0, code bit 1, N: 0.375 bytes per base) and one u64 offset per read.
 * on = 1 (capacity_bases_hint sizes the first allocation; 0: the first batch does): accepted only while the context
 *   holds no reads — freshly created or after shk_reset — otherwise SHK_ERR_STATE.  A retained read's index is its
 *   ordinal among the reads handed to the context since then, whatever shk_set_read_index says.  on = 0 frees the
 *   store, at any time.  shk_reset empties the store, keeps its allocation and leaves retention on; shk_destroy frees
 *   it.  Off by default.  A multi-device context refuses the call (SHK_ERR_STATE) unless it was created with
 *   SHK_FLAG_GROUP_READS: then on = 1 switches every device's store on (each with its share of the hint) under the same
 *   condition taken over the whole context, and a read's index is again its ordinal among the reads handed to the
 *   context, whichever device holds it.  What such a context retains: every batch of shk_ingest_reads / _batch, the
 *   room on every device reserved before the call's first round (SHK_ERR_NOMEM leaves the call undone).
 * WHAT IS RETAINED: every batch of shk_ingest_reads / _batch / _packed / _reads_device / _packed_device, on owner
 *   shares too (whole reads, not the share's k-mers), appended on the context's stream.  The exchange rounds (the
 *   shk_xchg_ scatter calls) retain nothing; shk_insert_counts and shk_insert_device add no reads.  The store grows
 *   geometrically; when room for a batch cannot be had the ingest returns SHK_ERR_NOMEM with nothing counted and
 *   nothing retained from that call.  An invalid byte poisons the context as without retention, and every retained
 *   call on a poisoned context returns that error. */
int shk_retain_reads(shk_ctx *ctx, int on, uint64_t capacity_bases_hint);
/* Reads and bases retained so far, and the device memory the store holds (0, 0, 0 with retention off); summed over the
 * devices of a multi-device context with SHK_FLAG_GROUP_READS. */
int shk_retained_info(shk_ctx *ctx, uint64_t *n_reads, uint64_t *n_bases, uint64_t *device_bytes);
/* Retained reads first_read .. first_read + n_reads as ASCII on the host (N where the read had one): offsets gets
 * n_reads + 1 entries from 0, *n_bases the total.  bases_cap too small: SHK_ERR_BAD_ARG with *n_bases set to the need
 * and nothing written.  Also SHK_ERR_BAD_ARG: a range beyond the retained reads; SHK_ERR_STATE: retention is off.
 * A multi-device context with SHK_FLAG_GROUP_READS: the same, the pieces of the range exported by the devices that hold
 * them and put together in order. */
int shk_retained_export(shk_ctx *ctx, uint64_t first_read, uint64_t n_reads, uint8_t *bases, uint64_t bases_cap,
                        uint64_t *offsets, uint64_t *n_bases);
/* shk_filter_reads_panel_device and shk_thread_reads_panel_device with the batch being every read retained so far, in
 * retention order: the same outputs, match_cap / link_cap protocol, limits, tuning and errors; read_index and mate take
 * one entry per retained read.  The walks read the planes as they lie — no byte loads, no ballots.  SHK_ERR_STATE
 * with retention off; zero retained reads: all-zero outputs.  They wait for every queued append, may be called in the
 * middle of a job (later ingests go on appending) and neither read nor write the table.
 * A multi-device context with SHK_FLAG_GROUP_READS answers with the same outputs, protocols and errors, indices being
 * the context's: every device walks its own store at the same time; the filter's lists are merged per gene into
 * ascending order; the threading's supports are added, its links summed by (in, out), read_edges written back to list
 * positions and n_paired_links counted on the host over all of them, so mates held by two devices pair up. */
int shk_filter_reads_panel_retained(shk_ctx *ctx, const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes,
                                    uint64_t *match_offsets, uint64_t *match_reads, uint64_t match_cap, uint64_t *n_matches);
int shk_thread_reads_panel_retained(shk_ctx *ctx, const uint64_t *node_sub_kmers, const uint64_t *node_offsets,
                                    const uint32_t *edge_src, const uint32_t *edge_tgt, const uint64_t *edge_offsets, uint32_t n_genes,
                                    const uint64_t *list_offsets, const uint64_t *list_reads,
                                    const uint64_t *read_index, const uint8_t *mate, shk_thread_panel_out *out);

/* The bulk neighbourhood of a seed set in sPCR's extension graph: every table lookup extend_graph
 * (src/pcr/graph.rs:377-525) can make from these seeds at this threshold, fetched breadth-first on the device, many
 * levels per launch.  For a context of k-mer length k ≥ 2, mask = (1 << 2(k−1)) − 1:
 *   node   a (k−1)-mer as a 2-bit value (DBNode.sub_kmer), ≤ mask;
 *   dir    bit 0 forward, bit 1 reverse; 3 stands for the two entries (node, F) and (node, R);
 *   the expansion of (s, F) is the four k-mers (s << 2) | b, of (s, R) the four (b << 2(k−1)) | s (graph.rs:419-423);
 *   x is ACCEPTED when the merged count c of min(x, revcomp(x)) — what shk_lookup(canonical = 1) returns — is
 *   ≥ min_count (0 is treated as 1); its successor, x & mask for F and x >> 2 for R, keeps the dir (graph.rs:441-444).
 * Level 0 is the set of distinct seed (node, dir) pairs; level i + 1 the distinct successors of level i's accepted
 * k-mers that are in no level ≤ i; K_L the distinct canonical k-mers accepted in the expansions of levels 0..L−1.
 * The call expands WHOLE levels: level L if and only if L < max_levels (0: no limit), level L is not empty, and
 * afterwards |K_{L+1}| ≤ cap and |level L+1| ≤ fringe_cap; otherwise it stops with level L unexpanded, and nothing of
 * a level that did not fit shows.  Out: K_L in kmers/counts ascending by k-mer (*n_out entries), level L in
 * fringe_nodes/fringe_dirs ascending by (node, dir) with one dir bit per entry (*n_fringe entries; 0 when the
 * neighbourhood is complete), *levels_done = L.  Calling again with the fringe as seeds continues the search (it may
 * report k-mers and entries again that an earlier call reported).  A deterministic function of table and arguments.
 * Errors: dir 0 or > 3, a node > mask, more distinct seeds than fringe_cap: SHK_ERR_BAD_ARG; a multi-device context
 * or an owner share (a neighbour's count may live on another share): SHK_ERR_STATE.  A multi-device context created
 * with SHK_FLAG_GROUP_GRAPH answers instead: the same search on its first device, every probe into the share that owns
 * the key; the result is that of one context holding the union of the shares.  Valid whenever shk_lookup is;
 * the table is not touched.  cap, fringe_cap ≤ 2^32; the device scratch is about 100 bytes per unit of cap.  The call
 * is one job of shk_neighborhood_panel (below): the same kernels and scratch layout, its lists fetched from the job's
 * own arrays instead of a packed copy. */
int shk_neighborhood(shk_ctx *ctx, const uint64_t *nodes, const uint8_t *dirs, uint64_t n_seeds,
                     uint32_t min_count, uint32_t max_levels,
                     uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n_out,
                     uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t fringe_cap, uint64_t *n_fringe,
                     uint32_t *levels_done);

/* create_seed_graph + extend_graph (src/pcr/graph.rs:196-528) under the threshold sweep of do_pcr
 * (src/pcr/mod.rs:559-619), replayed on the host statement for statement over counts that shk_neighborhood fetched
 * (defaults of the reference in brackets). */
typedef struct shk_pcr_extend_params {
  uint32_t min_count;          /* PCRParams.min_count [2]: the sweep's lowest threshold */
  uint32_t table_min_count;    /* FilteredKmerCounts' floor, cli --min-kmer-count [2] (counting.rs:306-345) */
  double   high_coverage_ratio;/* [10.0] graph.rs:495 */
  uint64_t max_num_nodes;      /* compute_node_budget(n_bases_ingested) or the caller's; graph.rs:389 */
  uint32_t sweep;              /* 1: thresholds of compute_coverage_thresholds (mod.rs:403-428), stop at the first
                                  step that finds a path (mod.rs:585-619); 0: one extension at min_count */
  uint32_t reserved;
} shk_pcr_extend_params;
/* fwd_/rev_kmers: the two primer k-mer sets as shk_primer_kmers returns them (primer at the 5' end); their counts
 * feed the sweep's min(max fwd, max rev) (mod.rs:542-562).  Out: the graph of the last step run (current_graph,
 * mod.rs:613) — nodes in NodeIndex order (sub_kmer, flags: 1 is_start, 2 is_end), edges in EdgeIndex order (source
 * and target node index, DBEdge.count) — *found_path of that step, its threshold, the steps run.  An empty set is not
 * an error (do_pcr returns before, mod.rs:446-468): the other set's seeds are extended and no path is found.
 * node_cap / edge_cap too small: SHK_ERR_BAD_ARG with *n_nodes / *n_edges set to what is needed.  A k-mer counts
 * when its merged count ≥ max(threshold, table_min_count, 1).  Multi-device contexts and owner shares:
 * SHK_ERR_STATE, as shk_neighborhood; a multi-device context with SHK_FLAG_GROUP_GRAPH answers, as shk_neighborhood.
 * The call is shk_pcr_extend_panel (below) for one gene, replayed on the calling thread; a host allocation that fails in the replay is SHK_ERR_NOMEM.  Tuning: SHK_PCR_FETCH_CAP (k-mers, read at
 * each call) bounds one neighbourhood fetch; the result does not depend on it.  The panel's own knobs
 * (SHK_PCR_PANEL_FETCH_CAP, SHK_PCR_PANEL_THREADS, SHK_PCR_PANEL_TRACE) do not apply to this call. */
int shk_pcr_extend(shk_ctx *ctx, const uint64_t *fwd_kmers, const uint32_t *fwd_counts, uint64_t n_fwd,
                   const uint64_t *rev_kmers, const uint32_t *rev_counts, uint64_t n_rev,
                   const shk_pcr_extend_params *p,
                   uint64_t *node_sub_kmers, uint8_t *node_flags, uint64_t node_cap, uint64_t *n_nodes,
                   uint32_t *edge_src, uint32_t *edge_tgt, uint32_t *edge_counts, uint64_t edge_cap, uint64_t *n_edges,
                   uint32_t *found_path, uint32_t *threshold_used, uint32_t *steps_run);
/* shk_neighborhood for many independent seed sets in ONE call: the table side of shk_pcr_extend_panel, where every gene
 * of a panel asks for the neighbourhood of its own queue at its own threshold (extend_graph, src/pcr/graph.rs:377-525,
 * once per gene of stats.rs:85-87).  Each job is carried through its levels by one workgroup of its own (a chain is as
 * deep as the amplicon is long and about one entry wide), so a panel's chains run side by side in the time of the
 * longest; a job whose level outgrows a workgroup is finished alone afterwards, a wide launch per level.
 * LAYOUT: job j's seeds are nodes/dirs[seed_offsets[j] .. seed_offsets[j+1]) (n_jobs + 1 offsets, non-decreasing); its
 *   k-mers and counts are written from index caps[0] + … + caps[j−1] of kmers/counts, its fringe from index
 *   fringe_caps[0] + … + fringe_caps[j−1] of fringe_nodes/fringe_dirs; n_out[j], n_fringe[j], levels_done[j].
 * RESULT: for every j exactly what shk_neighborhood returns on the same table for (j's seeds, min_counts[j],
 *   max_levels, caps[j], fringe_caps[j]) — the whole-levels rule, both lists sorted.  Jobs share nothing: each has its
 *   own two sets, entry lists and counters.  A job without seeds returns zeros; n_jobs == 0 is SHK_OK.
 * Errors, raised before the device is touched, with a text that names the job: every argument error of
 *   shk_neighborhood, decreasing seed_offsets: SHK_ERR_BAD_ARG; also n_jobs > SHK_PCR_MAX_GENES.  Multi-device
 *   contexts and owner shares: SHK_ERR_STATE; a multi-device context with SHK_FLAG_GROUP_GRAPH answers, with the
 *   launches of the one-device call (the share directory rides in the call's one upload).  Valid whenever shk_lookup is; the table is not touched.  The device
 *   scratch per job is 8 bytes × (the powers of two above 8·cap + 2·seeds and above 2·cap, for the two sets) plus 24
 *   bytes per unit of cap and 24 per unit of fringe_cap (lists and their packed copies): 140 to 210 bytes per unit of
 *   cap when fringe_cap = cap, the upper end at a power-of-two cap.  It is the context's grow-only scratch and stays
 *   with it; when it cannot be had the call fails with SHK_ERR_NOMEM and the context stays usable. */
#define SHK_PCR_MAX_GENES 4096   /* = SHK_FILTER_MAX_GENES = SHK_THREAD_MAX_GENES */
int shk_neighborhood_panel(shk_ctx *ctx, const uint64_t *nodes, const uint8_t *dirs,
                           const uint64_t *seed_offsets /* n_jobs + 1 */, uint32_t n_jobs,
                           const uint32_t *min_counts /* n_jobs */, uint32_t max_levels,
                           const uint64_t *caps, const uint64_t *fringe_caps /* n_jobs each */,
                           uint64_t *kmers, uint32_t *counts, uint64_t *n_out /* n_jobs */,
                           uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t *n_fringe /* n_jobs */,
                           uint32_t *levels_done /* n_jobs */);

/* shk_pcr_extend for a whole sPCR panel in ONE call: do_pcr builds and extends one graph per gene (stats.rs:85-87,
 * src/pcr/mod.rs:559-619, src/pcr/graph.rs:196-528); this call replays every gene's extension on the host in rounds and
 * fetches what all of them need from the table with one shk_neighborhood_panel call per round.
 * IN: primer_kmers / primer_counts / primer_offsets are the kmers / counts / offsets of shk_primer_kmers for primers
 *   ordered forward, reverse per gene: direction 2g is gene g's forward set, 2g + 1 its reverse set (2·n_genes + 1
 *   offsets, non-decreasing).  An empty set is no error, as in shk_pcr_extend.  params[g]: gene g's parameters.
 * OUT: for every g exactly what shk_pcr_extend returns for gene g's two sets and params[g]: nodes in NodeIndex order at
 *   node_offsets[g] .., edges in EdgeIndex order at edge_offsets[g] .. with endpoints LOCAL to the gene (0 = the gene's
 *   first node), found_path[g], threshold_used[g], steps_run[g] — the graph arrays are the input form of
 *   shk_thread_reads_panel and pass straight on.  node_cap / edge_cap too small: SHK_ERR_BAD_ARG with both offset
 *   arrays complete (their last entries are the need).  n_genes == 0: zero offsets.
 * Errors, SHK_ERR_BAD_ARG with a text that names the gene and the direction: a primer k-mer that is not a k-mer (before
 *   the device is touched), decreasing primer_offsets; also n_genes > SHK_PCR_MAX_GENES, k < 2.  Multi-device contexts
 *   and owner shares: SHK_ERR_STATE; a multi-device context with SHK_FLAG_GROUP_GRAPH answers, as
 *   shk_neighborhood_panel.  The table is not touched.
 * Tuning, all read at each call, none changes the result: SHK_PCR_PANEL_THREADS (default 8, clamped to 1..16) host threads replay
 *   the genes of a round (1: serial); SHK_PCR_PANEL_FETCH_CAP (k-mers, default 2^22; 140 to 210 bytes of device
 *   scratch each, see shk_neighborhood_panel: up to 0.9 GB at the default, kept by the context) is shared evenly by the jobs of a launch — a job gets at least 4 × its seeds and at most what its node budget
 *   leaves, and a round whose minimums exceed the budget is cut into several launches; SHK_PCR_FETCH_CAP, when set, is
 *   the capacity of every job, as for shk_pcr_extend.  SHK_PCR_PANEL_TRACE (set to anything): one line on stderr per
 *   call with its rounds and launches. */
int shk_pcr_extend_panel(shk_ctx *ctx, const uint64_t *primer_kmers, const uint32_t *primer_counts,
                         const uint64_t *primer_offsets /* 2·n_genes + 1 */, uint32_t n_genes,
                         const shk_pcr_extend_params *params /* n_genes */,
                         uint64_t *node_sub_kmers, uint8_t *node_flags, uint64_t *node_offsets /* n_genes + 1 */, uint64_t node_cap,
                         uint32_t *edge_src, uint32_t *edge_tgt, uint32_t *edge_counts, uint64_t *edge_offsets /* n_genes + 1 */, uint64_t edge_cap,
                         uint32_t *found_path, uint32_t *threshold_used, uint32_t *steps_run /* n_genes each */);
/* compute_node_budget (graph.rs:40-52): 100 000 nodes up to 150 Mbp ingested, 500 000 from 750 Mbp, linear between. */
uint64_t shk_pcr_node_budget(uint64_t n_bases_ingested);

/* The pruning stage of do_pcr for a whole sPCR panel in ONE call: remove_low_coverage_tips → reachability_pruning →
 * annotate_coverage_ratios (src/pcr/mod.rs:631-697; src/pcr/pruning.rs, src/pcr/graph.rs:533-546), between
 * shk_pcr_extend_panel and shk_thread_reads_panel.  One workgroup per gene on the device.
 * IN: the output of shk_pcr_extend_panel as it is (n_genes outputs of shk_pcr_extend concatenated will do as well):
 *   per-gene offsets (n_genes + 1 each, non-decreasing), edge endpoints LOCAL to the gene, flags 1 = is_start,
 *   2 = is_end.  k is the context's k.  node_sub_kmers is only carried through on the host and may be NULL (the
 *   output's node_sub_kmers is not written then).  params[g]: gene g's parameters.
 * SEMANTICS, per gene, exactly the reference:
 *   Degrees are edge counts (neighbors_directed(..).count() on a StableDiGraph): parallel edges count severally, a
 *     self-loop counts in both directions.
 *   Tip stage (stages bit 0; pruning.rs:19-95): median = median_via_select of all edge counts of the INPUT graph, 1.0
 *     without edges; min_tip = max(median × tip_coverage_fraction, 1.0), computed once.  Rounds run until one removes
 *     nothing.  In a round every surviving node that is neither start nor end and has out-degree 0 or in-degree 0 is
 *     judged on the graph as it stood at the START of the round, and all nodes judged removable leave together with
 *     their edges.  Out-degree 0: removable iff tip_length_backward < k and its largest incoming edge count (0 without
 *     one), as f64, is < min_tip; in-degree 0: the same with tip_length_forward and its outgoing counts; both degrees
 *     0: both tests.  tip_length_backward (:99-124) starts at 1; while the current node has exactly one incoming edge
 *     whose source has out-degree <= 1 and is not a start node, it steps to that source and adds 1.
 *     tip_length_forward (:128-149) is the mirror image with in-degree and is_end.
 *   Reachability (stages bit 1; :170-214), on what the tip stage left: keep exactly the nodes reachable forward from
 *     some surviving start node AND backward from some surviving end node.
 *   Annotation (graph.rs:533-546): median of the pruned graph's edge counts; coverage_ratio[e] = count / median when
 *     there is an edge and median > 0, otherwise every ratio is 0.0 (what get_dbedge left).
 * OUT: node_keep[v] for every input node (index as in the input arrays), always.  The compacted graphs: the surviving
 *   nodes and edges (an edge survives iff both endpoints do) in ascending original index at out_node_offsets[g] .. /
 *   out_edge_offsets[g] .., endpoints renumbered to positions in the compacted gene — the input form of
 *   shk_thread_reads_panel; node_index / edge_index: each survivor's original local index.  tip_rounds counts the
 *   rounds that removed something.  node_cap / edge_cap too small: SHK_ERR_BAD_ARG with both out-offset arrays (their
 *   last entries are the need), node_keep, median and the counters complete.  n_genes == 0: zero offsets.  An empty
 *   gene is valid; a gene without a start or an end prunes to nothing.
 * Errors, SHK_ERR_BAD_ARG with a text that names the gene, all raised before the device is touched: an endpoint >= the
 *   gene's node count, decreasing offsets, a flag above 3, a NaN tip_coverage_fraction, stages > 3; also n_genes >
 *   SHK_PCR_MAX_GENES and 2^32 or more nodes or edges in total.  Scratch that cannot be had: SHK_ERR_NOMEM, the context
 *   stays usable.
 * State: the table is neither read nor written; valid in any state of the context and on owner shares; a multi-device
 *   context runs it on its first device.  The kernel takes no slot of shk_timings: device_ms is the call's own.
 * Tuning, read at each call, never changes a result: SHK_PRUNE_LDS_NODES (default 2560) — a gene of at most that many
 *   nodes whose adjacency and state fit 79 KiB (24 bytes per node + 8.25 per edge) is pruned in LDS, larger ones in
 *   the context's grow-only scratch (16 bytes per node on top of the upload); 0: every gene in global memory. */
typedef struct shk_pcr_prune_params {
  double   tip_coverage_fraction; /* PCRParams.tip_coverage_fraction [0.1] */
  uint32_t stages;                /* bit 0 remove_low_coverage_tips, bit 1 reachability_pruning; 0 is read as 3 */
  uint32_t reserved;
} shk_pcr_prune_params;

typedef struct shk_pcr_prune_out {      /* every pointer optional except node_keep */
  uint8_t  *node_keep;                  /* [node_offsets[n_genes]] 1 = the node survives */
  uint64_t *out_node_offsets, *out_edge_offsets;  /* [n_genes + 1] */
  uint64_t *node_sub_kmers; uint8_t *node_flags; uint32_t *node_index; uint64_t node_cap;
  uint32_t *edge_src, *edge_tgt, *edge_counts, *edge_index; double *coverage_ratio; uint64_t edge_cap;
  double   *median;                     /* [n_genes] median edge count of the pruned graph, 0.0 when it has no edges */
  uint32_t *tip_rounds, *tips_removed, *unreachable_removed;  /* [n_genes] each */
  double    device_ms;                  /* event time of the call's launches */
} shk_pcr_prune_out;

int shk_pcr_prune_panel(shk_ctx *ctx, const uint64_t *node_sub_kmers, const uint8_t *node_flags, const uint64_t *node_offsets,
                        const uint32_t *edge_src, const uint32_t *edge_tgt, const uint32_t *edge_counts, const uint64_t *edge_offsets,
                        uint32_t n_genes, const shk_pcr_prune_params *params /* n_genes */, shk_pcr_prune_out *out);

/* ---- the last stage of do_pcr: paths, sequences, scores, dedup (src/pcr/mod.rs:699-813) ---- */

/* A panel's pruned graphs with their optional threading annotations, as the earlier stages emit them. */
typedef struct shk_pcr_graphs {
  uint32_t n_genes; uint32_t reserved;
  /* the output layout of shk_pcr_prune_panel: offsets n_genes + 1 each, endpoints LOCAL to the gene */
  const uint64_t *node_sub_kmers; const uint8_t *node_flags; const uint64_t *node_offsets;
  const uint32_t *edge_src, *edge_tgt, *edge_counts; const double *coverage_ratio; const uint64_t *edge_offsets;
  /* the layout of shk_thread_panel_out; all may be NULL (no gene has annotations then).  has_threading[g] != 0: gene g
   * was threaded (its read list was not empty, mod.rs:664-697); NULL with annotations present: every gene was. */
  const uint32_t *support_total, *support_unambiguous; const uint64_t *link_offsets;
  const uint32_t *link_in, *link_out, *link_counts; const uint8_t *has_threading;
} shk_pcr_graphs;

typedef struct shk_pcr_paths_params {  /* PCRParams, with the reference's defaults */
  uint64_t min_length, max_length;     /* [0] [10000] */
  uint64_t max_dfs_states;             /* [100000] */
  uint64_t max_paths_per_pair;         /* [20], counted per start node */
  uint64_t max_node_visits;            /* [2] */
} shk_pcr_paths_params;

#define SHK_PCR_SCORE_FIELDS 6  /* kmer_min_count, coverage_cv, max_coverage_ratio, zero_support_edges,
                                   median_unambiguous_support, edge_support_fraction; NaN stands for None */
typedef struct shk_pcr_records {        /* every pointer optional except record_offsets */
  uint64_t *record_offsets;             /* [n_genes + 1] gene g's records are [record_offsets[g], record_offsets[g+1]) */
  uint64_t *seq_offsets;                /* [record_cap + 1] record r's bases are seqs[seq_offsets[r] .. seq_offsets[r+1]) */
  uint8_t  *seqs;                       /* ASCII */
  uint64_t  record_cap, seq_cap;
  uint64_t  n_records, n_seq_bytes;     /* OUT: what the call produced — the need when a capacity was too small */
  uint32_t *start_node;                 /* per record: the path's first node, local to the gene */
  uint64_t *path_nodes;                 /* per record: nodes on the path */
  double   *count_mean, *count_median; uint64_t *count_min, *count_max;
  double   *score;                      /* PathScore::composite */
  double   *score_fields;               /* [SHK_PCR_SCORE_FIELDS per record] */
  uint64_t *paths_found, *generated, *states_explored;  /* [n_genes]: paths of get_assembly_paths, records of
                                           generate_sequences_from_paths, DFS pops summed over the gene's start nodes */
} shk_pcr_records;

/* resolve_bubbles → get_assembly_paths → generate_sequences_from_paths (pcr/bubble.rs:52-275, pcr/paths.rs:78-356) for
 * every gene of a panel, on the host (no context, no device: the search is one dependent chain), on a
 * few threads over genes (SHK_PCR_PANEL_THREADS, default 8, clamped to 1..16).
 * SEMANTICS, per gene, exactly the reference.  A node's outgoing (incoming) edges are taken newest first, i.e. in
 *   DESCENDING edge index: petgraph links a new edge at the head of its node's list and the pruning only removes.
 *   sorted_children visits by count × preference descending, equal scores in ASCENDING edge index (stable ascending
 *   sort, popped from the back).  Bubble preferences exist only for a gene with annotations: sources in ascending node
 *   index, branches along single-out-edge nodes for at most 50 steps, evidence = Σ support_total + Σ link_counts of
 *   (edge into the source, first edge) in wrapping u32, ranked by evidence descending then edge k-mer ascending,
 *   preference evidence / max (1.0 when max is 0), later writes replace earlier ones.  One search per start node in
 *   ascending node index; states_explored counts every pop; an end node at >= min_path_nodes is recorded and not
 *   extended, below it is walked through; the start node itself is never tested.  Records: the start node's (k-1)-mer
 *   plus one base per step; shorter than min_length or without edges: skipped.  Without annotations the three
 *   read-support fields are NaN (None) and the composite takes no read-support factor.
 * OUT: per gene the records in enumeration order.  record_cap / seq_cap too small: SHK_ERR_BAD_ARG with n_records,
 *   n_seq_bytes, record_offsets and the per-gene counters complete.
 * Errors, SHK_ERR_BAD_ARG with a text in err that names the gene: an endpoint >= the gene's node count, decreasing
 *   offsets, a flag above 3, k < 2 or k > 31, a sub-k-mer above the (k-1)-base mask, a link edge >= the gene's edge
 *   count, n_genes > SHK_PCR_MAX_GENES.  Host memory that cannot be had: SHK_ERR_NOMEM. */
int shk_pcr_paths_panel(uint32_t k, const shk_pcr_graphs *graphs, const shk_pcr_paths_params *params /* n_genes */,
                        shk_pcr_records *out, char *err, size_t err_cap);

/* 1 when the Levenshtein distance of a[0..la) and b[0..lb) is <= t, else 0: what bounded_levenshtein(a, b, t).is_some()
 * answers (paths.rs:388-391).  Banded two-row DP over bytes, any alphabet, any lengths, any t. */
int shk_edit_within(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb, uint32_t t);

#define SHK_PCR_MAX_AMPLICONS 20  /* MAX_NUM_AMPLICONS, paths.rs:20 */
typedef struct shk_pcr_dedup_out {      /* every pointer optional */
  uint32_t *kept;                       /* [SHK_PCR_MAX_AMPLICONS * n_genes] gene g's kept records at 20 g ..: indices
                                           into the gene's input records, in final order; returned[g] of them */
  uint32_t *generated, *retained, *returned;  /* [n_genes]: records in, kept before truncation, kept */
  uint32_t *order;                      /* [record_offsets[n_genes]] per gene: sorted position -> input index */
  uint64_t *pair_words;                 /* the within-t bits of all pairs i < j of the SORTED order, gene g's at word
                                           pair_offsets[g]: pair (i, j) of m records is bit i(2m-i-1)/2 + j-i-1 */
  uint64_t *pair_offsets;               /* [n_genes + 1], in 64-bit words */
  uint64_t  pair_cap;                   /* words of pair_words */
  uint64_t  pairs_device, pairs_host, pairs_prefiltered;  /* OUT: how the pairs were decided */
  double    device_ms;                  /* event time of the call's launch */
} shk_pcr_dedup_out;

/* sort_and_deduplicate (paths.rs:360-427) for every gene of a panel.  IN: gene g's records are
 * [record_offsets[g], record_offsets[g+1]); record r is the ACGT bytes seqs[seq_offsets[r] .. seq_offsets[r+1]) with
 * scores[r]; thresholds[g] is the gene's dedup_edit_threshold.  The host sorts each gene by score descending
 * (total_cmp) then bytes ascending; the within-t relation of ALL pairs of the sorted order is computed — by K_DEDUP on
 * the device (one lane per pair, Landau-Vishkin over 2-bit packed words), or by shk_edit_within on the
 * host for a gene with t > 31 or a record of 2^30 bases or more, and for the whole call when its pairs that need an
 * alignment number fewer than SHK_DEDUP_DEVICE_PAIRS (read at each call; 0 = always the device; never changes a
 * result).  Pairs with |la - lb| > t (0) or t >= max(la, lb) (1) need none.  Then greedily: a record is kept exactly
 * when no earlier KEPT record is within t; at most SHK_PCR_MAX_AMPLICONS are returned.  With SHK_TRACE set the call
 * prints one line to stderr: genes, pairs on the device, on the host, decided by the prefilters.
 * Errors: SHK_ERR_BAD_ARG naming the gene or record for decreasing offsets, a byte outside ACGT, n_genes >
 * SHK_PCR_MAX_GENES, pair_cap too small (pair_offsets complete).  Scratch that cannot be had: SHK_ERR_NOMEM, the context
 * stays usable.  State: as shk_pcr_prune_panel — the table is not touched, any state, owner shares, first device. */
int shk_pcr_dedup_panel(shk_ctx *ctx, const uint8_t *seqs, const uint64_t *seq_offsets, const uint64_t *record_offsets,
                        const double *scores, const uint32_t *thresholds, uint32_t n_genes, shk_pcr_dedup_out *out);

/* shk_pcr_paths_panel, then shk_pcr_dedup_panel with thresholds[g], then the renumbering of mod.rs:785-813: out holds
 * the final products per gene in product order 0, 1, .. (record_offsets[g+1] - record_offsets[g] of them); generated[g]
 * counts the records before the dedup, retained[g] (optional) those kept before the truncation.  k is the context's. */
int shk_pcr_products_panel(shk_ctx *ctx, const shk_pcr_graphs *graphs, const shk_pcr_paths_params *params,
                           const uint32_t *thresholds, shk_pcr_records *out, uint32_t *retained, double *device_ms);

/* ---- do_pcr / run_pcr: the stages above as one call over a panel (src/pcr/mod.rs:431-819, src/stats.rs:49-183;
 *      DESIGN.md §18) ---- */

typedef struct shk_pcr_gene {          /* PCRParams as do_pcr reads it; reference defaults in brackets */
  const char *gene_name, *forward_seq, *reverse_seq;   /* primers upper case IUPAC, as parse_pcr_primers_string leaves them */
  uint64_t min_length /*0*/, max_length /*10000*/;
  uint32_t min_count /*2*/, mismatches /*2*/, trim /*15*/, dedup_edit_threshold /*10*/;
  uint64_t max_dfs_states /*100000*/, max_paths_per_pair /*20*/, max_node_visits /*2*/;
  uint32_t max_primer_kmers /*40*/, reserved;
  double   high_coverage_ratio /*10.0*/, tip_coverage_fraction /*0.1*/;
} shk_pcr_gene;
/* The defaults of parse_pcr_primers_string (cli.rs:17-27, 131-136): everything but the three strings, which are left. */
void shk_pcr_gene_defaults(shk_pcr_gene *g);

/* parse_pcr_primers_string (cli.rs:12-140): "key=value,key=value,..." into *out (defaults first).  Items are split on
 * commas, each at its first '=', keys lower-cased; name, forward, reverse (upper-cased), max-length, min-length,
 * min-count, mismatches, trim, dedup-edit-threshold; citation and notes are accepted and dropped.  The three strings
 * are stored NUL-terminated in `strings` (strings_cap bytes; strlen(spec) + 3 always suffice) and *out points into it.
 * SHK_ERR_BAD_ARG with the reference's text in err (at most err_cap bytes with the NUL): "Invalid empty primer
 * specification", "Invalid parameter (should be key=value): '…'…", "Duplicate parameter '…' in primer specification
 * '…'. Each key may appear at most once.", "Unexpected parameter: …", and for a number that does not parse "Invalid
 * value for {key}: {value}" (the context anyhow prints first; its cause line is Rust's ParseIntError text and is not
 * reproduced). */
int shk_pcr_parse_primers(const char *spec, shk_pcr_gene *out, char *strings, size_t strings_cap, char *err, size_t err_cap);
/* validate_pcr_params (mod.rs:295-399): the number of (error, suggestion) pairs found, 0 for a valid gene; they are
 * written to buf as "error\nsuggestion\n" per pair in the reference's order (at most buf_cap bytes with the NUL; buf may
 * be NULL).  Host only, no context. */
int shk_pcr_validate_gene(const shk_pcr_gene *g, char *buf, size_t buf_cap);
/* The bail! text of collect_pcr_params (cli.rs:528-554) over n genes: returns the total number of errors (0: nothing
 * written), "Primer validation failed (N error[s]):\n" and per failing gene "\n  {name} ({source}):\n" with
 * "    - {error}\n      Suggestion: {suggestion}\n" lines.  sources[g] NULL (or sources NULL): "--pcr-primers". */
int shk_pcr_validation_report(const shk_pcr_gene *genes, uint32_t n, const char *const *sources, char *buf, size_t buf_cap);

#define SHK_PCR_SUCCESS 0u
#define SHK_PCR_NO_FORWARD 1u   /* "forward primer not found" (mod.rs:449-467) */
#define SHK_PCR_NO_REVERSE 2u   /* "reverse primer not found" */
#define SHK_PCR_NO_PRIMERS 3u   /* "forward and reverse primers not found" */
#define SHK_PCR_NO_PATH 4u      /* "no path found" (mod.rs:567) */
#define SHK_PCR_NODE_BUDGET 5u  /* "node budget exceeded" (mod.rs:621-623) */
/* PcrOutcome.failure_reason for a status: NULL for SHK_PCR_SUCCESS (and for a number that is no status). */
const char *shk_pcr_failure_reason(uint32_t status);

#define SHK_PCR_READS_NONE 0u      /* reads = None: k-mer-only scoring */
#define SHK_PCR_READS_RETAINED 1u  /* every read retained so far (shk_retain_reads) */
#define SHK_PCR_READS_HOST 2u      /* bases / offsets / n_seqs below, as shk_ingest_reads */
typedef struct shk_pcr_run_params {
  uint32_t min_kmer_count;   /* cli --min-kmer-count [2]: FilteredKmerCounts' floor; 0 is read as 1 */
  uint32_t reads;            /* SHK_PCR_READS_* */
  uint32_t paired;           /* RETAINED or HOST without read_index/mate: reads alternate R1, R2, index = ordinal
                                (reread_sequences, io.rs:831-898); 0: every read Unpaired */
  uint32_t reserved;
  uint64_t max_num_nodes;    /* 0: shk_pcr_node_budget(n_bases_ingested of the context) (main.rs:147-165) */
  const uint8_t *bases; const uint64_t *offsets; uint64_t n_seqs;
  const uint64_t *read_index; const uint8_t *mate;   /* HOST only, both or neither; given, they override `paired` */
  uint64_t reserved2[4];
} shk_pcr_run_params;

typedef struct shk_pcr_run_out {   /* every pointer optional except records.record_offsets and status; [n_genes] each */
  shk_pcr_records records;         /* the final products of all genes in gene order: the layout and the capacity
                                      protocol of shk_pcr_products_panel (a gene without products has none) */
  uint32_t *status;                /* SHK_PCR_* */
  uint32_t *n_fwd_kmers, *n_rev_kmers;       /* sizes of the two primer k-mer sets */
  uint32_t *max_fwd_count, *max_rev_count;   /* get_max_count of each (mod.rs:542-543); 0 for an empty set */
  uint32_t *median_primer_count;   /* min of the two get_median_count (mod.rs:546-548, counting.rs:275-298) */
  uint32_t *threshold_used, *steps_run, *found_path;  /* shk_pcr_extend_panel's; 0 for a gene that returned before */
  uint64_t *n_nodes, *n_edges;     /* of the extended graph (the last step run) */
  uint64_t *n_pruned_nodes, *n_pruned_edges;  /* of the pruned graph; 0 without a found path */
  uint64_t *n_reads_matched;       /* the gene's filter list length; 0 without reads */
  uint8_t  *threaded;              /* 1: the gene's reads were threaded through its pruned graph (mod.rs:664-697) */
  uint64_t *n_paired_links;        /* thread_reads_paired's paired_links.len() */
  uint8_t  *low_primer_counts;     /* 1: either max count below 5 (mod.rs:752-759) */
  uint64_t reserved[4];
} shk_pcr_run_out;

/* run_pcr's loop over do_pcr (stats.rs:84-98, mod.rs:431-819) for a panel, the genes side by side: every stage above is
 * called ONCE for all genes still alive, and not at all when none is left.  Needs a finalized context, as
 * shk_primer_kmers.  Per gene, in this order:
 *   1. min_count <- max(min_count, min_kmer_count) (collect_pcr_params, cli.rs:556-570).
 *   2. shk_primer_kmers for the whole panel (forward then reverse per gene; min_count the clamped one, max_kmers =
 *      max_primer_kmers).  An empty set: status 1 / 2 / 3 and nothing more for the gene (mod.rs:446-468).
 *   3. With reads: the gene's filter set is the canonical forms of both sets (from_primer_kmers, read_filter.rs:24-41);
 *      one panel filter pass for the genes that got this far.
 *   4. shk_pcr_extend_panel with min_count, table_min_count = min_kmer_count, high_coverage_ratio, max_num_nodes, sweep.
 *   5. The reason starts as NO_PATH; the last step's graph with n_nodes >= max_num_nodes makes it NODE_BUDGET
 *      (mod.rs:621, path or not).
 *   6. Only with found_path: prune (tip_coverage_fraction); thread iff reads were given and the gene's list is not empty
 *      (mod.rs:664-697), paired iff some listed read has mate != 0 (mod.rs:671); shk_pcr_products_panel with annotations
 *      exactly for the threaded genes.  At least one generated record: SUCCESS; otherwise the reason of step 5 stays.
 * READS: a HOST batch is staged once for both read-side stages; RETAINED runs both over the planes (SHK_ERR_STATE with
 *   retention off); with `paired` and no arrays the mate of read i is 1 + (i & 1) and its index i, looked up for listed
 *   reads only.  Zero reads behave like an empty list for every gene.
 * ERRORS, the first gene in gene order that has one, with a text that names the gene, all before the device is touched;
 *   within a gene: its first shk_pcr_validate_gene failure, then "Duplicate gene name '…'" when an earlier gene has the
 *   name (cli.rs:572-581), both SHK_ERR_BAD_ARG; then get_primer_kmers' errors in its order — too many variants
 *   forward, reverse, invalid character forward, reverse (primers.rs:440-478; the validation lets no character through
 *   that the conversion refuses).  Multi-device contexts and owner shares: SHK_ERR_STATE, as shk_pcr_extend_panel.
 *   A multi-device context with SHK_FLAG_GROUP_GRAPH answers for SHK_PCR_READS_NONE and SHK_PCR_READS_HOST: the primer
 *   scan over its shares, the extension as shk_pcr_extend_panel, the host batch staged once on its first device, where
 *   the filter, the threading, the prune and the products run.  Created with SHK_FLAG_GROUP_READS as well, and reads
 *   retained, it answers for SHK_PCR_READS_RETAINED too: the filter and the threading run over every device's store as
 *   shk_filter_reads_panel_retained / shk_thread_reads_panel_retained do there; without that flag it retains no reads
 *   (SHK_PCR_READS_RETAINED: "reads are not retained").  The result is the one-device context's, array for array.
 *   records.record_cap / seq_cap too small: SHK_ERR_BAD_ARG with n_records / n_seq_bytes the need and every per-gene
 *   array complete.  n_genes == 0: SHK_OK, nothing launched.
 * With SHK_TRACE set: one line per gene on stderr after the run. */
int shk_pcr_run(shk_ctx *ctx, const shk_pcr_gene *genes, uint32_t n_genes, const shk_pcr_run_params *params,
                shk_pcr_run_out *out);

/* ---- sPCR depth sweep -------------------------------------------------------------------------------
 * The table keeps one count lane per chunk, so the cumulative table at every chunk boundary is still there after
 * shk_finalize.  On a context with n_chunks lanes (shk_counters.n_chunks), DEPTH d, 1 ≤ d ≤ n_chunks, is the table of
 * chunks 0..d−1 merged: a key's count is the saturating sum of lanes 0..d−1 in lane order, and a key whose sum is 0 is
 * not in that table.  Depth n_chunks is the merged table.  Every call below returns, for a depth d, what its plain form
 * returns on a context that was handed only the reads of chunks < d — array for array, orders, level_hits, error texts
 * and the capacity protocols included; hence wherever the plain form accepts count ≥ min_count, the depth form accepts
 * the depth's count ≥ max(min_count, 1).
 * ERRORS common to all of them, before the device is touched: SHK_ERR_BAD_ARG for a depth 0 or above n_chunks (a list:
 * also n_depths 0 or above SHK_PCR_MAX_DEPTHS, or not strictly ascending); SHK_ERR_STATE on a multi-device context
 * (SHK_FLAG_GROUP_GRAPH or not), on an owner share, and between shk_xchg_scatter_begin and _end.  Valid whenever the
 * plain form is; the table is not written. */
#define SHK_PCR_MAX_DEPTHS 16
/* Chunk::n_bases of every chunk (n_chunks entries): shk_counters.n_bases_ingested is their sum.  After shk_finalize. */
int shk_chunk_bases(shk_ctx *ctx, uint64_t *n_bases_ingested);
/* shk_lookup at a depth. */
int shk_lookup_depth(shk_ctx *ctx, const uint64_t *kmers, uint32_t *counts, uint64_t n, int canonical, uint32_t depth);
/* shk_primer_kmers at n_depths depths in ONE pass over the table: the mismatch levels of a (k-mer, primer) pair are
 * computed once, whatever the number of depths.  Result slot j · n_primers + i is primer i at depths[j]: offsets has
 * n_depths · n_primers + 1 entries, level_hits (optional) n_depths · n_primers × SHK_PRIMER_LEVELS, and depth j's block
 * (slots j · n_primers .., offsets rebased) is exactly a shk_primer_kmers result.  cap ≥ n_depths · Σ max_kmers; also
 * n_depths · n_primers < 2^24.  SHK_PRIMER_CANDIDATES: on an overflow the cut level is per (primer, depth). */
int shk_primer_kmers_depths(shk_ctx *ctx, const shk_primer *primers, uint32_t n_primers, const uint32_t *depths,
                            uint32_t n_depths, uint64_t *kmers, uint32_t *counts, uint8_t *levels, uint64_t cap,
                            uint64_t *offsets, uint64_t *level_hits);
/* shk_neighborhood_panel with one depth per job (jobs of different depths share the launches); all else identical. */
int shk_neighborhood_panel_depths(shk_ctx *ctx, const uint64_t *nodes, const uint8_t *dirs,
                                  const uint64_t *seed_offsets, uint32_t n_jobs, const uint32_t *min_counts,
                                  const uint32_t *job_depths, uint32_t max_levels, const uint64_t *caps,
                                  const uint64_t *fringe_caps, uint64_t *kmers, uint32_t *counts, uint64_t *n_out,
                                  uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t *n_fringe,
                                  uint32_t *levels_done);
/* shk_pcr_extend_panel with one depth per gene; all else identical (tuning variables, round cutting, outputs). */
int shk_pcr_extend_panel_depths(shk_ctx *ctx, const uint64_t *primer_kmers, const uint32_t *primer_counts,
                                const uint64_t *primer_offsets, uint32_t n_genes, const shk_pcr_extend_params *params,
                                const uint32_t *gene_depths, uint64_t *node_sub_kmers, uint8_t *node_flags,
                                uint64_t *node_offsets, uint64_t node_cap, uint32_t *edge_src, uint32_t *edge_tgt,
                                uint32_t *edge_counts, uint64_t *edge_offsets, uint64_t edge_cap, uint32_t *found_path,
                                uint32_t *threshold_used, uint32_t *steps_run);
/* shk_pcr_run (reads = SHK_PCR_READS_NONE) of the panel at every listed depth, as ONE pipeline over the
 * n_genes · n_depths (gene, depth) pairs — pair j · n_genes + g is gene g at depths[j]: one fused primer scan, one
 * shk_pcr_extend_panel_depths over the pairs with both primer sets, one prune, one products call; a stage with no pair
 * left is not called.  outs[j] (n_depths of them, each with its own arrays and record capacities) is shk_pcr_run's
 * result at depths[j].  max_num_nodes 0: shk_pcr_node_budget(Σ chunk bases below the depth), per depth.  The host
 * checks run once per gene, in shk_pcr_run's order.  Record capacities: per outs[j]; on a short return
 * (SHK_ERR_BAD_ARG) every outs[j] has its need and its per-gene arrays complete.
 * ERRORS beyond the common ones: n_genes · n_depths > SHK_PCR_MAX_GENES; params->reads != SHK_PCR_READS_NONE
 * ("a depth sweep takes no reads": the store does not keep a read's chunk) — SHK_ERR_BAD_ARG. */
int shk_pcr_run_depths(shk_ctx *ctx, const shk_pcr_gene *genes, uint32_t n_genes, const shk_pcr_run_params *params,
                       const uint32_t *depths, uint32_t n_depths, shk_pcr_run_out *outs);

/* The owner of a canonical k-mer among n_owners shares, as the engine assigns it (shk_config.n_owners, the shares of a
 * multi-device context): the top log2(n_owners) bits of the key mix of the 2k-bit value.  Host only, no context: what a
 * multi-process job routes a query by.  n_owners: a power of two ≤ 64 (1: always 0).  ~0u for k = 0, k ≥ 32 or an
 * n_owners that is none. */
uint32_t shk_key_owner(uint32_t k, uint32_t n_owners, uint64_t canonical_kmer);

/* ---- multi-GPU hooks (device pointers; exchanged by the caller over RCCL) ---- */

/* Table geometry needed to shard by owner: n_pages (power of two),
 * page_slots, n_lanes.  Pages [p0,p1) are contiguous in every array. */
int shk_table_geometry(shk_ctx *ctx, uint64_t *n_pages, uint32_t *page_slots,
                       uint32_t *n_lanes);
/* Grow the table until it has at least n_pages pages (all ranks must agree
 * before exchanging page ranges). */
int shk_table_reserve_pages(shk_ctx *ctx, uint64_t n_pages);
/* Device pointers to the live table arrays: keys u64[n_pages*page_slots],
 * vals u32[n_lanes][n_pages*page_slots]. Valid until the next growing call. */
int shk_table_device_ptrs(shk_ctx *ctx, void **d_keys, void **d_vals);
/* KmerCounts::extend across devices (counting.rs:157-166): merge a peer's
 * page range [p0,p1) (same geometry; device pointers to its keys and to its
 * lane-major vals for that range, lane l at d_vals + l*vals_lane_stride u32
 * elements) into this table, saturating per lane. */
int shk_merge_pages(shk_ctx *ctx, uint64_t p0, uint64_t p1, const void *d_keys,
                    const void *d_vals, uint64_t vals_lane_stride);
/* The same merge with only the OCCUPIED entries on the wire.  The table's pages split evenly over
 * n_owners contiguous ranges (owner o = pages [o·P/n, (o+1)·P/n)).
 *   shk_owner_counts   : counts[o] = occupied slots of owner o's range
 *   shk_compact_owners : writes owner o's entries to d_keys[seg_offsets[o] ..] (and lane l of their
 *                        counts to d_vals + l·vals_lane_stride + the same index), owner after owner;
 *                        skip_owner ≥ 0: that owner's range is left out (a rank keeps its own)
 *   shk_merge_entries  : KmerCounts::extend (counting.rs:157-166) of n received entries */
int shk_owner_counts(shk_ctx *ctx, uint32_t n_owners, uint64_t *counts);
int shk_compact_owners(shk_ctx *ctx, uint32_t n_owners, const uint64_t *seg_offsets, void *d_keys, void *d_vals,
                       uint64_t vals_lane_stride, int32_t skip_owner);
int shk_merge_entries(shk_ctx *ctx, const void *d_keys, const void *d_vals, uint64_t n, uint64_t vals_lane_stride);
/* shk_compact_owners with every owner's entries as ONE self-contained piece of d_buf — at byte offset
 * (Σ_{o'<o} counts[o'])·(8 + 4·n_lanes): [k-mers 8·c][lane 0 counts 4·c] … [lane L−1 counts], c = counts[o]
 * (from shk_owner_counts; counts[skip_owner] must be 0) — so that k-mers and all lanes' counts cross the links
 * in one all-to-all.  A received piece goes to shk_merge_entries(piece, piece + 8·c, c, c).  Asynchronous on
 * the context's stream (shk_stream). */
int shk_compact_owners_packed(shk_ctx *ctx, uint32_t n_owners, const uint64_t *counts, void *d_buf, int32_t skip_owner);
/* The same (the sender's half of KmerCounts::extend across devices, counting.rs:157-166) with pieces of a FIXED
 * capacity (entries) at fixed places, so that nobody has to know anybody's counts
 * before the all-to-all (no host read-back in front of it).  Piece o lies at byte offset o·(8 + capacity·(8 +
 * 4·n_lanes)): an 8-byte header, then [k-mers][lane 0]…[lane L-1] with unused places holding EMPTY k-mers (all
 * ones).  Entries beyond the capacity are NOT written; the header of every piece holds how many entries the
 * fullest owner range of this sender had.  Asynchronous on the context's stream. */
int shk_compact_owners_fixed(shk_ctx *ctx, uint32_t n_owners, uint64_t capacity, void *d_buf, int32_t skip_owner);
/* KmerCounts::extend (counting.rs:157-166, saturating per lane as counting.rs:144-149) of the n_pieces received
 * fixed-capacity pieces lying back to back (what the equal-split
 * all-to-all of shk_compact_owners_fixed buffers delivers, this rank's own piece included at skip_piece) in ONE
 * launch.  All or nothing: if ANY header says a range had more entries than the capacity, nothing is merged —
 * every rank receives a piece from every sender, so every rank decides alike — and the caller repeats the exchange
 * with exact counts (shk_owner_counts / shk_compact_owners_packed).  Asynchronous like shk_merge_entries;
 * shk_merge_pieces_max reports the largest header seen (valid after the next shk_finalize or shk_sync):
 * > capacity ⇒ nothing was merged. */
int shk_merge_pieces(shk_ctx *ctx, const void *d_buf, uint32_t n_pieces, uint64_t capacity, int32_t skip_piece);
int shk_merge_pieces_max(shk_ctx *ctx, uint64_t *max_count);
/* The owned range of shk_set_owned_pages — the part of the merged table (io.rs:1023-1028) whose histogram this
 * context contributes — as share `owner` of `n_owners` (a power of two) equal parts of the pages,
 * worked out when the histogram scan is launched — so it needs no look at the table geometry (which would have to
 * wait for the counting launches) and follows the table when a merge grows it. */
int shk_set_owner_share(shk_ctx *ctx, uint32_t n_owners, uint32_t owner);
/* Restrict finalize's histogram scan to pages [p0,p1) (owner shard). */
int shk_set_owned_pages(shk_ctx *ctx, uint64_t p0, uint64_t p1);

/* ---- key-space-partitioned ingest: the exchange between owner shares (device pointers) -------------
 *
 * One round, on every one of the W contexts (cfg.n_owners = W, cfg.owner_id = its rank):
 *   1. shk_xchg_scatter_device: the rank's batch (≤ SHK_XCHG_MAX_BASES bases, resident in HBM) is
 *      validated, its canonical k-mers (kmers_from_ascii, encoding.rs:332-371) extracted and their 4-byte
 *      records written, grouped by owner, into the context's exchange buffer: owner o's SEGMENT is
 *      d_records + o·layout.segment_records (u32 records) with its fill levels at d_cursors + o·layout.regions
 *      (u32 words) — one contiguous piece each, so "send every peer its segment" is one all-to-all with
 *      equal splits (or W−1 peer copies).  The context has TWO exchange buffers and takes them in turn: what a
 *      call hands out stays valid until the next call BUT ONE, so round r's segments can be on the links while
 *      round r + 1 is scattered.  The call returns when the kernel is done: *n_foreign_spilled
 *      is the fill of the context's foreign spill list (records that overflowed a region on skewed input;
 *      shk_xchg_spill), an invalid byte is reported here (SHK_ERR_INVALID_CHAR) and poisons the context.
 *   2. the caller moves segment o to rank o (RCCL all_to_all / hipMemcpyPeer), rank r's own segment
 *      needs no copy;
 *   3. shk_xchg_absorb on every received segment (and the own one): level-2 partition of its records into
 *      the context's (lane, page) regions, where they wait for the page pass like any deferred batch.
 *      Asynchronous on the context's stream (shk_stream): the segment must stay untouched until the
 *      stream has passed the call.
 * Foreign spills: shk_xchg_spill exposes the list (k-mer, chunk lane, count triples of any owner);
 * every rank hands every other rank's list to shk_insert_device (which drops what the context does
 * not own) and then calls shk_xchg_spill_clear.  All of it is exact for any input.
 * Needs 4-byte records at the exchange geometry: 2k − layout.log_p1 ≤ 32 (k ≤ 21 at the default
 * fan-out of 1024); otherwise SHK_ERR_STATE — take the wide round (shk_xchg_wide_scatter_device below) or merge
 * the tables at finalize instead (shk_merge_*). */
#define SHK_XCHG_MAX_BASES (1ull << 28)
typedef struct shk_xchg_layout {
  uint32_t n_owners;        /* W */
  uint32_t n_lanes;         /* chunk lanes (max(chunks, 1)) */
  uint32_t log_p1;          /* level-1 fan-out bits, owner bits included */
  uint32_t regions;         /* regions per owner segment: n_lanes << (log_p1 − log2 W), ordered [lane][super-page] */
  uint32_t region_cap;      /* records per region (a multiple of 1024); 4-byte records: the regions of a segment are
                               block-interleaved — record j of region g at ((j>>10)·regions + g)<<10 | (j & 1023); 8-byte
                               records: region g at g·region_cap, linear */
  uint32_t record_bytes;    /* 4: the low bits of the mixed key below the level-1 fan-out (2k − log_p1 ≤ 32: k ≤ 21);
                               8 (round 4): the canonical k-mer itself (k ≥ 18 on a two-level table) — runs are padded to
                               even length with the all-ones word; 0 reads as 4 */
  uint64_t segment_records; /* regions · region_cap */
} shk_xchg_layout;
/* layout_bases: what the segments are sized for — every rank of a round passes the same number
 * (≥ its n_bases; e.g. the round's batch size), so that all come out with the same layout; 0 = n_bases.
 * The layout is a function of the configuration and of layout_bases, never of a table's size: a share is created with
 * at least the level-1 fan-out's pages over all owners, so layout.log_p1 is the fan-out on every share from shk_create
 * on, and a share whose table has grown scatters and absorbs the same segments as a peer whose table has not — no
 * caller has anything to do about a peer's growth (tests/test_gpu_share_sequences.py: route `grew_alone`). */
int shk_xchg_scatter_device(shk_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs,
                            uint64_t n_bases, uint64_t layout_bases, void **d_records, void **d_cursors,
                            shk_xchg_layout *layout, uint64_t *n_foreign_spilled);
/* The same scatter in two calls (round 4), for a caller that has something to put on the context's stream while the
 * scatter runs — the absorbs of the previous round's segments: _begin launches and returns at once, with the
 * segments' addresses and layout (functions of the configuration, not of the data), _end waits for the scatter
 * and reports what shk_xchg_scatter_device reports at its return (SHK_ERR_INVALID_CHAR and the poisoned context,
 * *n_foreign_spilled).  The segments are complete when _end has returned.  BETWEEN THE TWO the copy of the statistics
 * is pending and the scatter's outcome has not been looked at; what stays allowed on the context is
 *   shk_xchg_absorb, shk_reset (the round is given up), shk_destroy,
 *   and the calls that touch neither the device nor the job's state: shk_last_error, shk_stream, shk_xchg_feasible,
 *   shk_abi_version, shk_key_owner (shk_alloc_device and shk_free_device, which answer no code, are not looked at).
 * Every other entry point that takes the context returns SHK_ERR_STATE, "an exchange scatter is begun and not ended
 * (shk_xchg_scatter_end)", and leaves the context as it was but for that text: the _end that follows reports what it
 * would have reported and the round completes exactly.
 * With the one-call form the GPU stood idle every round from the end of the scatter until the host had woken up
 * and launched the absorbs (io.rs has no counterpart: it is the counting loop's batch boundary, io.rs:340-361). */
int shk_xchg_scatter_begin(shk_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs,
                           uint64_t n_bases, uint64_t layout_bases, void **d_records, void **d_cursors,
                           shk_xchg_layout *layout);
int shk_xchg_scatter_end(shk_ctx *ctx, uint64_t *n_foreign_spilled);
int shk_xchg_absorb(shk_ctx *ctx, const void *d_records, const void *d_cursors, const shk_xchg_layout *layout);
int shk_xchg_spill(shk_ctx *ctx, void **d_kmers, void **d_lanes, void **d_counts, uint64_t *n);
int shk_xchg_spill_clear(shk_ctx *ctx);
/* The exchange round for k-mers the owner layout cannot take (4-byte records need 2k − layout.log_p1 ≤ 32: k ≤ 21 at
 * the default fan-out; ≤ 128 chunk lanes) — any k, any number of lanes, slower: the batch is validated, its canonical
 * k-mers (kmers_from_ascii, encoding.rs:332-371) are extracted as whole 64-bit values and grouped by owner:
 *   *d_kmers u64[Σ counts], owner o's k-mers at [Σ_{o'<o} counts[o'], …) in no particular order;
 *   *d_lanes u32[Σ counts], each k-mer's chunk lane (read i → lane (i / 1000) % n_chunks, io.rs:340-361);
 *   counts   u64[n_owners], on the host.
 * The caller moves owner o's piece of both arrays to rank o (all-to-all with these split sizes) and every rank hands
 * what it receives to shk_insert_device with d_counts = NULL (one occurrence each: KmerCounts::ingest_seq's
 * saturating add, counting.rs:82-85, by device-scope atomics).  The call returns when the arrays are complete; an
 * invalid byte is reported here (SHK_ERR_INVALID_CHAR) and poisons the context.  The arrays stay valid until the next
 * scatter call on the context.  shk_xchg_feasible: 1 when the owner-layout rounds (shk_xchg_scatter_device) can take
 * this context's batches at its present table geometry, 0 when only the wide round can. */
int shk_xchg_wide_scatter_device(shk_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs,
                                 uint64_t n_bases, void **d_kmers, void **d_lanes, uint64_t *counts);
int shk_xchg_feasible(shk_ctx *ctx);
/* KmerCounts::insert (counting.rs:152-154) from device memory with a chunk lane per record:
 * saturating add of d_counts[i] to d_kmers[i] in lane d_lanes[i]; k-mers the context does not own
 * are dropped; d_counts = NULL: one occurrence each.  A count of 0 creates the entry all the same, as
 * shk_insert_counts does (a key with merged count 0 sits in no histogram bin: io.rs:1127-1132 then fails finalize).
 * Synchronous. */
int shk_insert_device(shk_ctx *ctx, const void *d_kmers, const void *d_lanes, const void *d_counts, uint64_t n);
/* The context's HIP stream (hipStream_t): device work queued by the calls above is ordered on it, so
 * a host that runs its collectives on the same stream needs no host-side synchronisation. */
void *shk_stream(shk_ctx *ctx);

/* ---- pinned staging buffers for streaming hosts -------------------------------- */
void *shk_alloc_pinned(size_t bytes);
void shk_free_pinned(void *p);
void *shk_alloc_device(shk_ctx *ctx, size_t bytes);
void shk_free_device(shk_ctx *ctx, void *p);
/* Blocks of device and pinned host memory that a context (or shk_free_pinned) gives back are kept by the process —
 * a bounded amount: 4 GiB per process on the devices, 512 MiB pinned, no block above 1 GiB / 160 MiB — and handed to
 * the next request of about their size: mapping and unmapping memory is what setting a context up and taking it down
 * costs (17-19 ms of an 80 ms FASTQ job).  This call gives everything back to the driver; the environment variable
 * SHK_NO_MEM_CACHE=1 turns the keeping off.  (The reference has no counterpart: its allocator is the process's.) */
void shk_release_cached_memory(void);

/* ---- synthetic reads, generated on device ------------------------ */

typedef struct shk_synth {
  uint64_t seed_genome;   /* 0x5EED0001 */
  uint64_t seed_reads;    /* 0x5EED0002 */
  uint64_t genome_len;    /* G */
  uint32_t read_len;      /* 150 */
  uint32_t sub_per_64k;   /* substitution errors per 65536 bases (0 = error-free) */
  uint32_t n_per_64k;     /* N per 65536 bases */
  uint32_t reserved;
} shk_synth;
/* Writes reads [first_read, first_read+n_reads) as ASCII to d_bases
 * (n_reads*read_len bytes) and offsets to d_offsets (n_reads+1 u64). */
int shk_synth_reads_device(shk_ctx *ctx, const shk_synth *spec, uint64_t first_read,
                           uint64_t n_reads, void *d_bases, void *d_offsets);

/* ---- host side either side of the path --------------------------------- */

/* FASTQ(.gz) front-end: read_fastq / open_fastq_reader / validate_fastq_record
 * (io.rs:161-198, 271-352, 598-625).  Parses only; state (read count, validation cadence,
 * --max-reads) persists across files like FastqReadState (io.rs:498-512).  n_paths == 0 reads
 * stdin (io.rs:517-537).  Errors carry the reference's texts (shk_fastq_error). */
typedef struct shk_fastq shk_fastq;
int shk_fastq_open(const char *const *paths, uint32_t n_paths, uint64_t max_reads,
                   uint64_t validate_every, shk_fastq **out);
/* The same with flags.  SHK_FASTQ_GZIP_ALL_MEMBERS: NOT what the reference does — its flate2::read::GzDecoder
 * (io.rs:606-617) reads a gzip file's FIRST member and stops, which is what shk_fastq_open does too; a bgzip'd FASTQ
 * or `cat a.fastq.gz b.fastq.gz` then counts as its first member (64 KB of a bgzip file).  With the flag every member
 * is read, the way flate2::read::MultiGzDecoder would: what follows a member's trailer is the next member's header,
 * every member's CRC-32 and length are checked, an error in any of them is the stream's (same texts). */
#define SHK_FASTQ_GZIP_ALL_MEMBERS 1u
int shk_fastq_open_ex(const char *const *paths, uint32_t n_paths, uint64_t max_reads,
                      uint64_t validate_every, uint32_t flags, shk_fastq **out);
/* BGZF (bgzip) input decoded in batches: NOT defaults, and both imply SHK_FASTQ_GZIP_ALL_MEMBERS' semantics.  A bgzip'd
 * file is thousands of gzip members of at most 64 KiB whose headers carry their compressed size (the BC subfield) and
 * whose trailers carry their decoded size, so the members are independent jobs with known extents before a bit is
 * decoded.  Consecutive members with that framing (FLG exactly FEXTRA, a BC subfield, body and text ≤ 65536 bytes) are
 * decoded side by side — SHK_FASTQ_BGZF_BATCH: on the reader's host threads; SHK_FASTQ_BGZF_DEVICE: on a HIP device,
 * one wave per member (the text comes back to the host parser — unless SHK_FASTQ_DEVICE_PARSE, below, keeps it in device
 * memory and frames the records there).  Every member's CRC-32 and ISIZE are checked before a byte of it is parsed.  At the first member that is not framed so, or whose decode, CRC-32 or ISIZE fails, the
 * one-after-the-other decoder of SHK_FASTQ_GZIP_ALL_MEMBERS takes over from that member's header on: reads, order,
 * errors and their texts are that flag's, whatever the file holds.  Flags 0 and 1 behave, and run, as before. */
#define SHK_FASTQ_BGZF_BATCH 2u
#define SHK_FASTQ_BGZF_DEVICE 4u
/* shk_fastq_open_ex with the device the SHK_FASTQ_BGZF_DEVICE route runs on (shk_fastq_open_ex: device 0).  With that
 * flag set and no such device to open — or in a build of the front-end alone — the call fails with SHK_ERR_NO_DEVICE
 * and a text in shk_run_error(); it never decodes on the host instead. */
int shk_fastq_open_device(const char *const *paths, uint32_t n_paths, uint64_t max_reads,
                          uint64_t validate_every, uint32_t flags, int device_id, shk_fastq **out);
/* gzip members decoded so far, by route: on the device, in host batches, one after the other (any may be NULL).  Ahead
 * of what has been handed out: the decoders run in front of the parse. */
int shk_fastq_member_stats(const shk_fastq *r, uint64_t *n_members_device, uint64_t *n_members_host_batch,
                           uint64_t *n_members_sequential);
/* Process-wide totals of the device route since the library was loaded (for measurements): members decoded, the
 * decode kernel's time in nanoseconds (hipEvents around its launches), bytes uploaded and bytes downloaded. */
int shk_bgzf_device_totals(uint64_t *n_members, uint64_t *kernel_ns, uint64_t *bytes_up, uint64_t *bytes_down);

/* ---- FASTQ text parsed on the device ----
 * shk_fastq_parse_device frames the records of n_bytes (at most 2^31) of FASTQ text that lies in device memory, at any
 * alignment, the way read_fastq / BufRead::lines / validate_fastq_record do (io.rs:161-198, 271-352): a line ends with
 * '\n', a '\r' directly in front of it is not part of the line; with `last` an unterminated rest is a line too (and
 * keeps a '\r' at its end); record j is lines 4j .. 4j+3.  The sequences go, concatenated, to d_bases and their offsets
 * to d_offsets[n_records + 1] — what shk_ingest_reads_device takes.  An ANOMALY is a record the host must decide about:
 * a byte >= 0x80 in one of its four lines, a sequence byte outside ACGTN, or, when the record's global index g =
 * first_record + j is validated (g == 0 || (validate_every && g % validate_every == 0)): a header that does not start
 * with '@', a separator that does not start with '+', a quality line of another length than the sequence.  The call
 * looks at records [0, min(whole records, max_records)) and emits those in front of the first anomaly among them;
 * bytes_consumed is where the last emitted record ends: what lies behind is the caller's (a partial record, fewer than
 * four lines, or the anomaly).  Synchronous.  SHK_ERR_BAD_ARG when a capacity is too small: out->n_records and
 * out->n_bases then say what the text needs (nothing is written beyond a capacity). */
#define SHK_FASTQ_ANOMALY_HIGH_BYTE 1u
#define SHK_FASTQ_ANOMALY_HEADER 2u
#define SHK_FASTQ_ANOMALY_SEPARATOR 3u
#define SHK_FASTQ_ANOMALY_QUALITY_LEN 4u
#define SHK_FASTQ_ANOMALY_BASE 5u   /* of several kinds in one record the lowest is reported */
typedef struct shk_fastq_text_params {
  uint64_t first_record;    /* global index of the text's first record (validation cadence) */
  uint64_t validate_every;
  uint64_t max_records;     /* emit at most this many; 0 = no limit */
  uint32_t last;            /* the text ends its file: an unterminated last line is a line */
  uint32_t reserved;
} shk_fastq_text_params;
typedef struct shk_fastq_text_result {
  uint64_t n_records, n_bases, bytes_consumed;
  uint64_t anomaly_record;  /* UINT64_MAX: none among the records looked at */
  uint32_t anomaly_kind, reserved;
} shk_fastq_text_result;
int shk_fastq_parse_device(shk_ctx *ctx, const void *d_text, uint64_t n_bytes, const shk_fastq_text_params *params,
                           void *d_bases, uint64_t bases_cap, void *d_offsets, uint64_t offsets_cap,
                           shk_fastq_text_result *out);
/* CRC-32 (gzip's) of n extents of d_text, one wave each: d_jobs[n] of shk_crc_job, d_crc[n] words (device pointers; an
 * extent of 0 bytes gives 0).  Synchronous. */
typedef struct shk_crc_job {
  uint64_t offset;
  uint32_t len, reserved;
} shk_crc_job;
int shk_crc32_members_device(shk_ctx *ctx, const void *d_text, const void *d_jobs, uint32_t n, void *d_crc);
/* The bytes of text one wave takes in the framing passes (tests put line ends on its borders). */
void shk_fastq_parse_geometry(uint32_t *tile_bytes);
/* The route: bgzip'd FASTQ files → the context, the text never leaving device memory.  Per batch of BGZF members the
 * compressed bytes go up, K_INFLATE decodes them, the members' CRC-32 are computed on the device and come down with the
 * statuses (8 bytes per member), the records are framed over carry + text, and the sequences are ingested
 * (shk_ingest_reads_device; retained if retention is on).  The read index, the cadence and max_reads run across the
 * files.  A single-device context that holds no reads (else SHK_ERR_STATE).
 * gave_up == 2: the input is not this route's (no path, a path that is no regular file, a first member that is not
 * BGZF, a multi-device context) — nothing was touched.  gave_up == 1: a member that is not BGZF, a decode status, a
 * CRC-32 or an anomaly in front of max_reads, a file that ends inside a record or without a final '\n', or a failure of
 * the route's own: the context
 * has been shk_reset (retention as it was) and the caller reads the whole input through shk_fastq_open*, whose reads,
 * errors and texts are then the outcome.  Both come with SHK_OK.  The route never decodes or parses on the host. */
typedef struct shk_fastq_device_stats {
  uint64_t n_batches, n_members;
  uint64_t n_records, n_bases;      /* framed on the device and ingested (= the context's reads when gave_up == 0) */
  uint64_t bytes_up, bytes_down;    /* the route's own traffic: compressed bytes and jobs up; statuses, CRCs, result words down */
  uint64_t kernel_ns;               /* the framing and CRC-32 kernels (hipEvents round their launches) */
  uint32_t gave_up, give_up_reason; /* reason: SHK_FASTQ_GIVEUP_* */
} shk_fastq_device_stats;
#define SHK_FASTQ_GIVEUP_NOT_ELIGIBLE 1u
#define SHK_FASTQ_GIVEUP_MEMBER 2u      /* a member that is not batchable BGZF */
#define SHK_FASTQ_GIVEUP_DECODE 3u      /* a decode status (a wrong ISIZE is one) */
#define SHK_FASTQ_GIVEUP_CRC 4u
#define SHK_FASTQ_GIVEUP_ANOMALY 5u
#define SHK_FASTQ_GIVEUP_TEXT_LEFT 6u   /* a file ends inside a record, or its last line has no '\n' */
#define SHK_FASTQ_GIVEUP_OWN 7u         /* a HIP error, an allocation, an ingest that failed, a carry beyond its room */
int shk_ingest_fastq_files_device(shk_ctx *ctx, const char *const *paths, uint32_t n_paths, uint64_t max_reads,
                                  uint64_t validate_every, shk_fastq_device_stats *out);
/* Process-wide totals of the route and of shk_fastq_parse_device / shk_crc32_members_device since the library was
 * loaded (any may be NULL): batches, records framed on the device, give-ups (gave_up != 0), bytes up, bytes down, the
 * framing and CRC-32 kernels' nanoseconds. */
int shk_fastq_device_totals(uint64_t *n_batches, uint64_t *n_records, uint64_t *n_give_ups, uint64_t *bytes_up,
                            uint64_t *bytes_down, uint64_t *kernel_ns);
/* shk_run_config.fastq_flags only, and only together with SHK_FASTQ_BGZF_DEVICE (alone: SHK_ERR_BAD_ARG): the run tries
 * shk_ingest_fastq_files_device first and, when that gives up, reads the input from the start with the flag cleared.
 * shk_fastq_open* refuse it (SHK_ERR_BAD_ARG): a reader hands out host batches. */
#define SHK_FASTQ_DEVICE_PARSE 8u
void shk_fastq_close(shk_fastq *r);
const char *shk_fastq_error(const shk_fastq *r);
/* Up to max_seqs sequences / bases_cap bytes, in input order; offsets[0] = 0.  A sequence that
 * does not fit is delivered first by the next call. */
int shk_fastq_next_batch(shk_fastq *r, uint8_t *bases, uint64_t bases_cap, uint64_t *offsets,
                         uint64_t max_seqs, uint64_t *n_seqs);
/* The same batch in the 2-bit packed input format (above: Read::from_str's layout over the batch's concatenated
 * bases + the N mask), packed while the sequences are copied out of the parsed file — what shk_pack_reads would make
 * of shk_fastq_next_batch's output, without the ASCII batch in between: packed takes (bases_cap+3)/4 bytes rounded up
 * to 8, nmask (bases_cap+31)/32 words; offsets are base indices from 0.  A byte outside ACGTN among the reads handed
 * out is SHK_ERR_INVALID_CHAR with the text of encoding.rs:353-356 (those reads are ones the reference would have
 * drained, io.rs:340-343, so it would have met the byte too). */
int shk_fastq_next_batch_packed(shk_fastq *r, uint8_t *packed, uint32_t *nmask, uint64_t bases_cap, uint64_t *offsets,
                                uint64_t max_seqs, uint64_t *n_seqs);
int shk_fastq_stats(const shk_fastq *r, uint64_t *n_reads_read, uint64_t *n_bases_read,
                    int *reached_max, int *done);

/* {sample}.histo / {sample}.final.histo, io.rs:1009-1014, 1051-1094 (byte for byte). */
int shk_write_histo(const char *path, const char *version, uint32_t k, uint32_t chunks,
                    uint64_t histo_max, const uint64_t *histo);
int shk_write_final_histo(const char *path, const char *version, uint32_t k, uint32_t chunks,
                          uint64_t histo_max, const uint64_t *histo);

/* RunStats (stats.rs:27-45) as filled at main.rs:182-197; pcr_results goes beside it (shk_write_stats_yaml_pcr). */
typedef struct shk_run_stats {
  const char *sharkmer_version;
  const char *command;
  const char *sample;
  uint32_t kmer_length;
  uint32_t chunks;
  uint64_t n_reads_read;
  uint64_t n_bases_read;
  uint64_t n_subreads_ingested;
  uint64_t n_bases_ingested;
  uint64_t n_kmers;
  uint64_t n_multi_kmers;      /* written only when has_histogram (chunks > 0) */
  uint64_t n_singleton_kmers;  /* idem */
  uint64_t peak_memory_bytes;  /* device memory in use at the end of the run */
  uint32_t has_histogram;
  uint32_t reserved;
} shk_run_stats;
int shk_write_stats_yaml(const char *path, const shk_run_stats *st); /* stats.rs:186-193 */

/* cli.rs:659-673 + 645-652: 0<k<32, k odd, 0<histo_max≤1e6, sample-name charset; the message is
 * available from shk_run_error(). */
int shk_validate_args(uint32_t k, uint64_t histo_max, const char *sample);
const char *shk_run_error(void);

/* ingest_reads + consolidate_and_histogram + write_stats over local files (main.rs:74-78,
 * 112-197 without sPCR; with it: shk_run_files_pcr below): the flags -k --chunks --histo-max -m -s -o --validate-every. */
typedef struct shk_run_config {
  const char *const *inputs; /* FASTQ(.gz) paths; n_inputs == 0 ⇒ stdin */
  uint32_t n_inputs;
  uint32_t k;
  uint32_t chunks;
  int32_t device;
  uint64_t histo_max;
  uint64_t max_reads;       /* 0 = all */
  uint64_t validate_every;  /* 0 = first record only */
  const char *sample;
  const char *outdir;       /* NULL = "./" */
  const char *command;      /* recorded in stats.yaml */
  const char *version;      /* NULL = "3.1.0" */
  uint64_t table_capacity_hint;
  uint64_t batch_reads;     /* reads per device super-batch; 0 = 1,000,000 */
  uint64_t batch_bases;     /* pinned buffer bytes; 0 = 256 MiB */
  uint32_t n_devices;       /* > 1: one multi-device context over device_ids (shk_config.n_devices); else `device` */
  uint32_t fastq_flags;     /* SHK_FASTQ_* (shk_fastq_open_ex); 0 = the reference's reader */
  const int32_t *device_ids;
} shk_run_config;
int shk_run_files(const shk_run_config *cfg, shk_run_stats *out_stats);

/* write_fasta_record (io.rs:144-158) for records first .. first + n of recs (the layout shk_pcr_run fills), the i-th of
 * them as product i: ">{sample}_{gene}_{i} sample={sample} gene={gene} product={i} length=… kmer_count_mean=…
 * kmer_count_median=… kmer_count_min=… kmer_count_max=… score=…" (paths.rs:331-343 as renumbered at mod.rs:785-813),
 * then the sequence wrapped at 80 columns (FASTA_LINE_WIDTH, io.rs:14).  The file is created or truncated. */
int shk_write_fasta(const char *path, const char *sample, const shk_pcr_gene *gene, const shk_pcr_records *recs,
                    uint64_t first, uint64_t n);

/* PcrGeneResult (stats.rs:11-23) as run_pcr fills it (stats.rs:102-145): status "success" for SHK_PCR_SUCCESS and
 * "fail" otherwise, failure_reason = shk_pcr_failure_reason(status); output_file is always None there. */
typedef struct shk_pcr_gene_stat {
  const char *gene_name;
  uint32_t status;                 /* SHK_PCR_* */
  uint32_t n_products;
  const uint64_t *product_lengths; /* [n_products]; the key is omitted when n_products == 0 */
} shk_pcr_gene_stat;
/* shk_write_stats_yaml plus pcr_results (stats.rs:43-44); n == 0 omits the key: the bytes of shk_write_stats_yaml. */
int shk_write_stats_yaml_pcr(const char *path, const shk_run_stats *st, const shk_pcr_gene_stat *results, uint32_t n);

/* The sPCR side of a file run: what --pcr-primers, --min-kmer-count, --read-threading and --node-budget-global set
 * (main.rs:133-178). */
typedef struct shk_pcr_file_config {
  const shk_pcr_gene *genes;
  uint32_t n_genes;
  uint32_t min_kmer_count;      /* [2]; 0 is read as 1 */
  uint32_t read_threading;      /* 1: retain the reads at ingest and thread them; stdin input: k-mer-only scoring
                                   (main.rs:136-139) */
  uint32_t dump;                /* reserved, 0 (--dump-graph is not built) */
  uint64_t node_budget_global;  /* 0 = shk_pcr_node_budget(n_bases_ingested) */
  uint64_t context_flags;       /* SHK_FLAG_* for the run's context: SHK_FLAG_GROUP_GRAPH, SHK_FLAG_GROUP_READS, both
                                   or 0, anything else is SHK_ERR_BAD_ARG (the first of what were four reserved words: same size and offsets) */
  const uint32_t *depths;       /* --pcr-depths: after the normal run, shk_pcr_run_depths at these depths (shk_pcr_check_depths
                                   holds) with {sample}_{gene}.depth{d}.fasta and {sample}.pcr_depths.tsv; NULL: no sweep */
  uint64_t n_depths;            /* (these two were reserved words: same size and offsets; more than SHK_PCR_MAX_DEPTHS go in
                                   several calls) */
  uint64_t reserved[1];
} shk_pcr_file_config;
/* shk_run_files with main.rs:133-199: after the histograms, shk_pcr_run over pcr->genes, {sample}_{gene}.fasta for every
 * gene with products in gene order (stats.rs:102-125), then the stats file with pcr_results.  A run that fails leaves no
 * stats file.  pcr NULL or without genes: shk_run_files.  out (optional) is handed to shk_pcr_run as it is: the caller's
 * arrays and capacities; NULL: the call keeps the products to itself.  n_devices > 1 with genes: SHK_ERR_STATE, unless
 * context_flags has SHK_FLAG_GROUP_GRAPH: then the run proceeds over the multi-device context; read_threading there
 * needs SHK_FLAG_GROUP_READS as well, and without it is SHK_ERR_STATE before a read is read (a multi-device context
 * keeps no reads). */
int shk_run_files_pcr(const shk_run_config *cfg, const shk_pcr_file_config *pcr, shk_run_stats *out_stats,
                      shk_pcr_run_out *out);

/* ---- the depth sweep of a file run (shk_count --pcr-depths) ----
 * With pcr->depths, shk_run_files_pcr runs shk_pcr_run_depths after the panel and writes, before the stats file,
 * {sample}_{gene}.depth{d}.fasta (shk_write_fasta) for every (gene, depth) with products and {sample}.pcr_depths.tsv.
 * Refused before a read is read (SHK_ERR_BAD_ARG, the text in shk_run_error()): no genes, read_threading, n_devices > 1,
 * chunks == 0, and what shk_pcr_check_depths refuses.  Every file of a run without depths is what it was. */
/* A depth list for a run of `chunks` chunks: n >= 1, every depth in 1..chunks, strictly ascending; else SHK_ERR_BAD_ARG
 * with the reason in err (at most err_cap bytes with the NUL). */
int shk_pcr_check_depths(const uint32_t *depths, uint64_t n, uint32_t chunks, char *err, size_t err_cap);
/* --pcr-depths' value: "all" (1..chunks) or "d1,d2,…" → depths[0 .. *n_depths), checked as above.  *n_depths is the
 * count also when it exceeds cap (SHK_ERR_BAD_ARG then, nothing beyond cap written). */
int shk_pcr_parse_depths(const char *spec, uint32_t chunks, uint32_t *depths, uint64_t cap, uint64_t *n_depths, char *err,
                         size_t err_cap);
typedef struct shk_pcr_depth_row {
  uint32_t depth;
  uint32_t reserved;
  uint64_t n_bases_ingested;       /* of the chunks below the depth */
  shk_pcr_gene_stat gene;
} shk_pcr_depth_row;
/* {sample}.pcr_depths.tsv: the header "depth n_bases_ingested gene status failure_reason n_products product_lengths"
 * (tab-separated), then one row per entry in the order given (the run: depth-major, then gene order); status "success"
 * or "fail", failure_reason empty on success, the lengths comma-separated (empty without products). */
int shk_write_pcr_depths_tsv(const char *path, const shk_pcr_depth_row *rows, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif
