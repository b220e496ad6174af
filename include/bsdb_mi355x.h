/*
 * bsdb_mi355x.h -- C ABI of the MI355X index-build hot path for bsdb.
 *
 * This is the boundary a JNI shim binds: plain pointers and
 * sizes, no JNI/torch types, int return codes (0 or a negative errno-style
 * code, mirroring src/main/c/native.c:29-34,54 where negative returns become
 * Java exceptions).  Reference paths below are relative to yc-huang/bsdb:
 *   W    = src/main/java/tech/bsdb/write/BSDBWriter.java
 *   CBHS = src/main/java/it/unimi/dsi/sux4j/io/ConcurrentBucketedHashStore.java
 *   GOV  = src/main/java/it/unimi/dsi/sux4j/mph/GOVMinimalPerfectHashFunctionModified.java
 *
 * Two families of entry points:
 *   bsdb_dev_*  operate on DEVICE pointers (HBM-resident keys) on a caller
 *               stream (hipStream_t passed as void*; NULL = the HIP null stream).
 *               Asynchronous: they enqueue and return.
 *   bsdb_*      (no dev_) take HOST pointers (a Java DirectByteBuffer / LBuffer
 *               address), stream them through the context's device staging
 *               buffers and return when the result is in host memory.
 *
 * Key layouts (W:75 put(byte[] key, ...) keys are 1..255 bytes, Common.java MAX_KEY_SIZE):
 *   fixed  n keys of key_len bytes, packed back to back (no padding).
 *   var    a byte blob of blob_bytes plus offsets[n+1] (u64); key i = blob[off[i] .. off[i+1]).
 *          No read goes past blob_bytes.
 *
 * Thread safety: calls on one context are serialised by the context's lock,
 * and the context orders its own work across streams: a call that uses the
 * context's workspace on a stream other than the previous call's first waits
 * (hipStreamWaitEvent) for the previous call's work.  put() is concurrent in
 * the reference (W:75, Builder.java:144-160); callers batch per thread and
 * submit through one shared context or one context per thread.
 *
 * Object handles (all opaque, passed to Java as jlong like native.c:50-59's
 * mph*, but every one has a matching free/close):
 *   bsdb_ctx    one HIP device: stream, workspace, host staging, RCCL rank
 *   bsdb_mph    a GOV MPHF resident on one device (E, 2-bit values, checksum bits)
 *   bsdb_index  the index.db / index_a.db writer of BSDBWriter.buildIndex
 *   bsdb_multi  one context per device of this process + an RCCL communicator
 *   bsdb_builder keys streamed into one device's HBM, built by bucket-range passes
 *   bsdb_db     a finished database resident on one device for batched gets:
 *               index.db and every kv.db partition in HBM; borrows its bsdb_mph
 */
#ifndef BSDB_MI355X_H
#define BSDB_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSDB_ABI_VERSION 6

/* Return codes (negative errno-style). */
#define BSDB_OK          0
#define BSDB_EINVAL    (-22)  /* bad argument (null pointer, key_len 0 or > 255, n too large) */
#define BSDB_ENOMEM    (-12)  /* device allocation failed                                  */
#define BSDB_EIO        (-5)  /* HIP runtime / kernel launch error                         */
#define BSDB_ENODEV    (-19)  /* no such HIP device                                        */
#define BSDB_EDUP      (-17)  /* duplicate 128-bit signature (CBHS:969-972, GOV:471-473)   */
#define BSDB_ESEEDS    (-34)  /* a bucket exhausted its 255 local seeds (GOV:431)          */
#define BSDB_ECOMM     (-70)  /* RCCL unavailable or a collective failed                   */
#define BSDB_EFILE     (-9)   /* file open/read/write failed (index / dump files)          */
#define BSDB_EVERIFY   (-74)  /* a built MPHF failed its on-device bijection check; a merge */
                              /* stopped on a damaged input (bsdb_db_merge)                 */

typedef struct bsdb_ctx bsdb_ctx;

int         bsdb_abi_version(void);
const char *bsdb_strerror(int code);

/* Opens a context on HIP device `device` (like Native.loadHash returning an
 * mph* as a jlong, native.c:50-59; unlike it, there is a matching close). */
int bsdb_open(int device, bsdb_ctx **out);
int bsdb_close(bsdb_ctx *ctx);

/* GOV:281,350-351 -- numBuckets = n/1500 + 1; multiplier = 2*numBuckets. */
uint64_t bsdb_num_buckets(uint64_t n);

/* ---------------------------------------------------------------------------
 * A3: per-key SpookyHash-short signature (sig0, sig1) = Hashes.spooky4(key, seed)
 * (CBHS:360-364 add(); in-tree C spec spooky.c:94-175).  d_sig receives 2n u64
 * (sig0, sig1 interleaved).  seed is the store seed (0 for BSDBWriter, CBHS:209).
 * Alignment: d_keys (fixed-length keys) and d_sig must be 16-byte aligned
 * (BSDB_EINVAL otherwise); d_blob may start at any address.
 * ------------------------------------------------------------------------- */
int bsdb_dev_hash_fixed(bsdb_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint64_t n,
                        uint64_t seed, uint64_t *d_sig, void *stream);
int bsdb_dev_hash_var(bsdb_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                      const uint64_t *d_offsets, uint64_t n, uint64_t seed, uint64_t *d_sig,
                      void *stream);

/* ---------------------------------------------------------------------------
 * A3+A4+A6 fused: hash -> bucket = multiplyHigh(sig0>>>1, 2*num_buckets)
 * (CBHS:900,965; GOV:559) -> bucket-occupancy histogram, ACCUMULATED into
 * d_counts[num_buckets] (u32).  Nothing per key is materialised in HBM beyond
 * a 2-byte partition id stream kept in the context workspace.  This is the
 * replacement for the producer loop GOV:385-402 (edgeOffsetAndSeed[b+1] =
 * edgeOffsetAndSeed[b] + bucket.size()).  Calling it once per key shard and
 * summing d_counts across devices (RCCL all-reduce) gives the global histogram.
 * Alignment: d_keys (fixed-length keys) must be 16-byte aligned (BSDB_EINVAL
 * otherwise); d_blob may start at any address.
 * ------------------------------------------------------------------------- */
int bsdb_dev_histogram_fixed(bsdb_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint64_t n,
                             uint64_t seed, uint64_t num_buckets, uint32_t *d_counts, void *stream);
int bsdb_dev_histogram_var(bsdb_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                           const uint64_t *d_offsets, uint64_t n, uint64_t seed,
                           uint64_t num_buckets, uint32_t *d_counts, void *stream);

/* A6: E[0] = 0, E[b+1] = E[b] + counts[b] (GOV:391-393), u64, m+1 entries.
 * The low 56 bits of edgeOffsetAndSeed; seeds are OR-ed in by the solver. */
int bsdb_dev_edge_offsets(bsdb_ctx *ctx, const uint32_t *d_counts, uint64_t num_buckets,
                          uint64_t *d_E, void *stream);

/* ---------------------------------------------------------------------------
 * MPHF evaluation over a solved GOV structure (sux4j layout, GOV:292-313):
 *   d_E       edgeOffsetAndSeed[num_buckets+1] (offset | local seed << 56)
 *   d_values  the 2-bit value array (LongArrayBitVector words, LSB first)
 *   d_sigbits the hash.checksum.bits list (width bits per rank), or NULL when width = 0
 * A12 (GOV:557-569, mph.c:86-96): out[i] = rank of signature i, or -1 when the
 * rank is >= n or the checksum bits differ (check != 0); check == 0 returns the
 * unchecked rank (GOV:573-580).
 * A11 (GOV:492-508): OR-s sig0 & mask(width) into d_sigbits at each key's rank
 * (d_sigbits zeroed by the caller, ceil(n*width/64)+1 words).
 * A13 (W:129-145): for records whose rank lies in [start, start+len):
 * index[rank-start] = byte-reversed addr (REVERSE_ORDER, Common.java:61); with
 * d_index_a, also the first min(value_len, 8) bytes of value8 (index.approximate).
 * Alignment: d_sig of bsdb_dev_lookup and bsdb_dev_sign must be 16-byte
 * aligned (a signature is read as one 16-byte pair; BSDB_EINVAL otherwise).
 * ------------------------------------------------------------------------- */
int bsdb_dev_lookup(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t nq, uint64_t n, uint64_t num_buckets,
                    const uint64_t *d_E, const uint64_t *d_values, uint32_t width,
                    const uint64_t *d_sigbits, int check, int64_t *d_out, void *stream);
int bsdb_dev_sign(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t n, uint64_t num_buckets,
                  const uint64_t *d_E, const uint64_t *d_values, uint32_t width, uint64_t *d_sigbits,
                  void *stream);
int bsdb_dev_index_scatter(bsdb_ctx *ctx, const int64_t *d_rank, const uint64_t *d_addr, uint64_t count,
                           uint64_t start, uint64_t len, uint64_t *d_index, const uint64_t *d_value8,
                           const uint8_t *d_value_len, uint8_t *d_index_a, void *stream);

/* ---------------------------------------------------------------------------
 * A5 + A6 + A8 + A11 on the device: GOV MPHF over n signatures (any order).
 * Buckets are sorted by unsigned (sig0, sig1) (CBHS:939-955), duplicates
 * rejected (BSDB_EDUP, CBHS:969-972), every bucket solved with local seeds
 * 0..255 (BSDB_ESEEDS when exhausted, GOV:431), values written with 3 for a
 * zero hinge (GOV:126-139), and, for width > 0, the checksum list signed
 * (GOV:492-508).  Outputs: d_E[num_buckets+1], d_values[bsdb_values_words(n)],
 * d_sigbits[(n*width+63)/64 + 1] (zeroed here).  The solution choice is this
 * project's deterministic solver (bit-identical to oracle/bo_gov_build), not
 * sux4j's; synchronous (returns after the device finished).
 * Alignment: d_sig of every bsdb_dev_gov_build* call must be 16-byte aligned
 * (BSDB_EINVAL otherwise).
 * ------------------------------------------------------------------------- */
#define BSDB_E2BIG     (-7)   /* a bucket holds more keys than the solver supports */
uint64_t bsdb_values_words(uint64_t n);
int bsdb_dev_gov_build(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t n, uint32_t width, uint64_t *d_E,
                       uint64_t *d_values, uint64_t *d_sigbits, void *stream);

/* F2: the same build, also returning d_rank[i] = the rank (getLong) of d_sig[i],
 * computed inside the solve (E[b] + the hinge vertices before the key's hinge:
 * the lookup's nonzero-pair count, GOV:557-580) -- no lookup pass over the
 * keys is needed to place records in index.db (W:129-145).  The
 * checksum bits are always signed this way (A11 fused into the solve). */
int bsdb_dev_gov_build_ranks(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t n, uint32_t width, uint64_t *d_E,
                             uint64_t *d_values, uint64_t *d_sigbits, int64_t *d_rank, void *stream);
/* E4: the same build restricted to the buckets [b_lo, b_hi) of a GOV structure
 * over n_global keys (one rank of the multi-GPU build).  d_sig
 * holds exactly the n_local signatures whose bucket lies in the range (any
 * order); e_lo = keys in buckets below b_lo.  d_E (num_buckets(n_global)+1),
 * d_values (bsdb_values_words(n_global)) and d_sigbits ((n_global*width+63)/64
 * + 1) are FULL-size arrays zeroed by the caller; the call writes E[b_lo..b_hi)
 * (plus E[m] on the last range), the 2-bit fields of the range's vertices and
 * the checksum fields of its ranks, and nothing else.  Fields of different
 * ranges are disjoint bits, so summing the ranks' arrays (one RCCL all-reduce
 * or reduce, ncclSum) assembles the global structure.  d_rank (optional):
 * the global rank of each of the n_local signatures, as bsdb_dev_gov_build_ranks. */
int bsdb_dev_gov_build_range(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t n_local, uint64_t n_global,
                             uint64_t b_lo, uint64_t b_hi, uint64_t e_lo, uint32_t width, uint64_t *d_E,
                             uint64_t *d_values, uint64_t *d_sigbits, int64_t *d_rank, void *stream);
/* E4 with O(n/G) memory per rank (ABI 6): the same range build into windows
 * of the structure instead of full-size arrays.  d_E_win holds E[b_lo..b_hi]
 * (b_hi - b_lo + 1 entries; E[b_hi] is zeroed again unless b_hi == m, as
 * above); d_values_win the value words [values_w0, values_w0 + values_words);
 * d_sigbits_win the checksum words [sig_w0, sig_w0 + sig_words) -- all zeroed
 * by the caller, and covering the words the range writes, which
 * bsdb_gov_range_windows gives as {values_w0, values_words, sig_w0, sig_words}
 * (BSDB_EINVAL otherwise).  A word shared with the next or the previous range
 * holds only this range's bits: the structure is the windows OR-ed at their
 * positions (distributed.py's assembly on rank 0). */
int bsdb_gov_range_windows(uint64_t n_global, uint32_t width, uint64_t e_lo, uint64_t n_local, uint64_t *out4);
int bsdb_dev_gov_build_window(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t n_local, uint64_t n_global,
                              uint64_t b_lo, uint64_t b_hi, uint64_t e_lo, uint32_t width, uint64_t *d_E_win,
                              uint64_t *d_values_win, uint64_t values_w0, uint64_t values_words,
                              uint64_t *d_sigbits_win, uint64_t sig_w0, uint64_t sig_words, int64_t *d_rank,
                              void *stream);
/* The whole build of a key set resident in this device's HBM (C4: 13.19e9 x
 * 13 B; C5: 4e9 var-len) by sequential bucket-range passes: pass p of P covers
 * buckets [p*m/P, (p+1)*m/P) (the reference's 256 spill segments are such
 * ranges, CBHS:379-395, solved one at a time, CBHS:852-978 / GOV:385-448).
 * Every pass re-hashes all keys and keeps its range's: no signature array for
 * the whole set.  Writes d_E / d_values / d_sigbits (sizes as
 * bsdb_dev_gov_build; zeroed here) and, optionally, index.db's slots
 * (W:129-145): slot rank(key i) = byte-reversed addr(i), addr(i) = d_addr[i]
 * when d_addr != NULL, else addr_base + addr_stride * i (fixed-size records of
 * one data file).  The slots go to d_index[n] (device) or h_index[n] (host
 * memory: each pass's contiguous slice is copied out while the next pass
 * solves) or nowhere when both are NULL.  passes = 0 picks the fewest passes
 * that fit the free HBM; *passes_used (optional) returns the count.  Results
 * equal bsdb_dev_gov_build's on the same keys.  Synchronous. */
int bsdb_dev_mph_build_index_passes_fixed(bsdb_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint64_t n,
                                          uint32_t width, uint32_t passes, const uint64_t *d_addr, uint64_t addr_base,
                                          uint64_t addr_stride, uint64_t *d_E, uint64_t *d_values, uint64_t *d_sigbits,
                                          uint64_t *d_index, uint64_t *h_index, uint32_t *passes_used, void *stream);
int bsdb_dev_mph_build_index_passes_var(bsdb_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes,
                                        const uint64_t *d_off, uint64_t n, uint32_t width, uint32_t passes,
                                        const uint64_t *d_addr, uint64_t addr_base, uint64_t addr_stride,
                                        uint64_t *d_E, uint64_t *d_values, uint64_t *d_sigbits, uint64_t *d_index,
                                        uint64_t *h_index, uint32_t *passes_used, void *stream);
/* E4 ownership: rank g of `nranks` owns buckets [g*m/nranks, (g+1)*m/nranks)
 * (m = num_buckets; the bucket is monotone in sig0, CBHS:129-138).  Groups the n
 * signatures of d_sig by owning rank into d_out (rank 0's first; order within a
 * rank unspecified) together with one u64 payload per key (the record address
 * of the index stage; d_payload / d_payload_out may be NULL), and writes the
 * per-rank counts to h_counts[nranks] (synchronises).  d_sig and d_out must be
 * 16-byte aligned (BSDB_EINVAL otherwise). */
int bsdb_dev_partition_owners(bsdb_ctx *ctx, const uint64_t *d_sig, const uint64_t *d_payload, uint64_t n,
                              uint64_t num_buckets, int nranks, uint64_t *d_out, uint64_t *d_payload_out,
                              uint64_t *h_counts, void *stream);
/* Frees the context's grown workspace (histogram id stream, GOV build
 * buffers, host staging): a long-lived context hands its HBM back between
 * builds (the next call grows what it needs again).  Synchronises the device. */
int bsdb_release_workspace(bsdb_ctx *ctx);
/* Debug/test option: after every GOV build, look every key up again on the
 * device and check the ranks form a permutation of [0, n) (BSDB_EVERIFY if not). */
int bsdb_set_verify(bsdb_ctx *ctx, int enable);

/* Histogram path selection for bsdb_dev_histogram_* (benchmarks/tests):
 *   0 = auto, 1 = partitioned two-pass, 2 = direct atomics,
 *   3 = single pass (13-byte keys on a 256-CU device, m <= 9 436 672 buckets,
 *       >= 4 * 256 * 16384 keys, <= 16384 keys per bucket on average: bucket owners per CU, ids exchanged through an
 *       on-die ring; other key sets, and the tail past its whole super-tiles,
 *       take the two-pass path).  Results are identical in every mode. */
int bsdb_set_histogram_mode(bsdb_ctx *ctx, int mode);
/* Key-load front end (for comparison runs; results are identical):
 * 0 = auto: 13-byte keys by the persistent binned kernel (dword-aligned
 *     16-byte windows), variable-length keys by the persistent binned kernel
 *     with per-wave LDS staging of 128-key groups;
 * 1 = the one-tile-per-workgroup kernel with LDS-staged sub-tiles;
 * 2 = the one-tile-per-workgroup kernel with direct reads. */
int bsdb_set_frontend(bsdb_ctx *ctx, int frontend);
/* Two-pass path, 13-byte keys: pass 2 of chunk i runs beside pass 1 of chunk
 * i + 1 (two id buffers; pass 2 keeps `p2_cus` CUs, pass 1 the rest; the
 * first pass 1 and the last pass 2 use the whole chip).  mode -1 = default,
 * 0 = serial chunks, 1 = pipelined; chunks / p2_cus 0 = defaults (8 chunks,
 * CUs / 8).  Results are identical either way. */
int bsdb_set_pipeline(bsdb_ctx *ctx, int mode, uint64_t chunks, uint32_t p2_cus);
/* Keys per pass-1 launch (chunk) of the partitioned path (0 = default);
 * rounded down to whole tiles of the pass-1 kernel.  The launches of a span
 * (the whole call, memory permitting) append to one set of id regions sized
 * for the span, and pass 2 runs once per span: the launch length changes
 * neither the workspace nor what pass 2 reads, only how pass 1 is cut into
 * launches.  Results are identical for every value. */
int bsdb_set_chunk_keys(bsdb_ctx *ctx, uint64_t chunk_keys);
/* Chunks the partitioned path recounted with direct atomics since open
 * because a partition region or LDS bin overflowed (adversarial key sets,
 * e.g. many duplicates).  Synchronises the device.  0 for normal inputs. */
int bsdb_fallback_count(bsdb_ctx *ctx, uint64_t *out);
/* Single-pass histogram (mode 3): launches enqueued since open, and those
 * whose bounded waits timed out (a workgroup never became resident; nothing
 * was added and the keys were recounted).  Synchronises the device. */
int bsdb_fused_status(bsdb_ctx *ctx, uint64_t *launches, uint64_t *timeouts);

/* Live per-kernel timing with HIP events recorded on the launch stream around
 * every pass-1 (hash+partition) and pass-2 (partition histogram) launch.
 * bsdb_profile_read synchronises those events and returns, for `kind`
 * (0 = pass 1, 1 = pass 2, 2 = edge-offset scan, 3 = the value compare of
 * bsdb_dev_db_check, k_check_values alone, 4 = the text kernel of
 * bsdb_dev_db_dump_text, k_dump_text alone, 5 = the value compare of
 * bsdb_dev_db_diff, k_diff_values alone, 6 = the image pack of
 * bsdb_dev_db_pack, k_rec_pack<true> or k_rec_pack_blocked alone; keys = records), the summed milliseconds, the
 * number of launches and the keys they processed; then clears that kind. */
int bsdb_set_profiling(bsdb_ctx *ctx, int enable);
int bsdb_profile_read(bsdb_ctx *ctx, int kind, double *total_ms, uint64_t *launches, uint64_t *keys);

/* ---------------------------------------------------------------------------
 * Host-buffer entry points (what the JNI shim calls with DirectByteBuffer
 * addresses).  Keys are copied H2D through pinned staging in the context;
 * counts are accumulated into the host array h_counts[num_buckets].
 * ------------------------------------------------------------------------- */
int bsdb_histogram_fixed(bsdb_ctx *ctx, const uint8_t *h_keys, uint32_t key_len, uint64_t n,
                         uint64_t seed, uint64_t num_buckets, uint32_t *h_counts);
int bsdb_hash_fixed(bsdb_ctx *ctx, const uint8_t *h_keys, uint32_t key_len, uint64_t n,
                    uint64_t seed, uint64_t *h_sig);
/* Variable-length keys in host memory, as BSDBWriter.put receives them
 * (byte[] of 0..255 bytes, kLen u8, BaseKVWriter.java:44-49): key i is
 * h_blob[h_off[i] .. h_off[i+1]), h_off[0..n] non-decreasing.  Same results
 * as bsdb_dev_{histogram,hash}_var on the same bytes; the keys are copied H2D
 * in batches of <= 256 MiB of key bytes (offsets rebased per batch). */
int bsdb_histogram_var(bsdb_ctx *ctx, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n,
                       uint64_t seed, uint64_t num_buckets, uint32_t *h_counts);
int bsdb_hash_var(bsdb_ctx *ctx, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n,
                  uint64_t seed, uint64_t *h_sig);

/* Synthetic SURVEY.md §8(d) D2 13-byte keys for indices [first, first+n),
 * written on device (benchmark input generator; not part of the build path).
 * d_keys must be 16-byte aligned (BSDB_EINVAL otherwise); exactly 13 n bytes
 * are written. */
int bsdb_dev_gen_keys13(bsdb_ctx *ctx, uint64_t first, uint64_t n, uint8_t *d_keys, void *stream);

/* Config C5 synthetic var-len keys: lengths 8..64 drawn
 * Zipf(1.1), bytes 0-7 = i big-endian, splitmix tail.  Writes d_offsets[n+1]
 * (offsets[0] = 0); with d_blob != NULL also the key bytes, after checking
 * offsets[n] <= blob_cap (synchronises).  Bench/test input generator only. */
int bsdb_dev_gen_keys_var(bsdb_ctx *ctx, uint64_t first, uint64_t n, uint64_t *d_offsets, uint8_t *d_blob,
                          uint64_t blob_cap, void *stream);

/* ---------------------------------------------------------------------------
 * B4: the one collective of the histogram stage, inside
 * this library.  RCCL is loaded at first use (dlopen librccl.so.1; BSDB_ECOMM
 * when absent).  Per-process ranks (one JVM or one torchrun rank per GPU):
 * rank 0 creates the 128-byte id, the host ships it to the other ranks over
 * its own channel, every rank calls bsdb_comm_init with it.
 * bsdb_dev_histogram_finalize then all-reduces the local counts over xGMI --
 * packed as u16 pairs (m/2 u32 words, 17.6 MB at C4), redone as u32 only if a
 * count does not fit -- and scans them into E[0..m] (every rank the same E);
 * it checks E[m] == n_total (synchronises; BSDB_ECOMM on mismatch).  d_counts
 * holds the global counts afterwards.
 * ------------------------------------------------------------------------- */
#define BSDB_COMM_ID_BYTES 128
/* 1 when this process can load RCCL (every rank should agree on it before
 * bsdb_comm_init, which is collective and waits for every rank), else 0. */
int bsdb_comm_available(void);
int bsdb_comm_unique_id(uint8_t *id /* [BSDB_COMM_ID_BYTES] */);
int bsdb_comm_init(bsdb_ctx *ctx, int nranks, int rank, const uint8_t *id);
int bsdb_dev_histogram_finalize(bsdb_ctx *ctx, uint32_t *d_counts, uint64_t num_buckets, uint64_t n_total,
                                uint64_t *d_E, void *stream);
/* Sum-all-reduce of u64 words on the context's communicator (assembles the
 * disjoint fields of bsdb_dev_gov_build_range outputs; BSDB_ECOMM without one). */
int bsdb_dev_allreduce_u64(bsdb_ctx *ctx, uint64_t *d_buf, uint64_t count, void *stream);

/* ---------------------------------------------------------------------------
 * B4: all the devices of one process (the reference's build runs in ONE JVM,
 * SURVEY.md §2.1), one bsdb_ctx per device and an RCCL communicator over them
 * (ncclCommInitAll, created by the first histogram call; the full build below
 * does not use it).  devices == NULL means 0..ndev-1.  The host-buffer calls
 * shard the keys in input order over the devices (one host thread per device,
 * each copying over its own PCIe link), histogram the shards, all-reduce the
 * counts with ONE collective and return E[0..m] (u64, offsets only) in h_E.
 * ------------------------------------------------------------------------- */
typedef struct bsdb_multi bsdb_multi;
int bsdb_multi_open(int ndev, const int *devices, bsdb_multi **out);
int bsdb_multi_close(bsdb_multi *mc);
int bsdb_multi_size(const bsdb_multi *mc);
int bsdb_multi_ctx(bsdb_multi *mc, int i, bsdb_ctx **out);
int bsdb_multi_histogram_fixed(bsdb_multi *mc, const uint8_t *h_keys, uint32_t key_len, uint64_t n, uint64_t seed,
                               uint64_t *h_E);
int bsdb_multi_histogram_var(bsdb_multi *mc, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n,
                             uint64_t seed, uint64_t *h_E);
/* E4: the whole build over every device of the process --
 * the single-device F2 call bsdb_mph_build_index_* with the key set sharded
 * over the devices.  Device g owns the buckets [g*m/G, (g+1)*m/G) (a sig0
 * range, CBHS:129-138; buckets are independent, GOV:405-448): each device
 * hashes its input-order shard, groups the signatures (and the records' addr /
 * value8 / vlen) by owner, ONE device-to-device exchange delivers them (xGMI
 * peer copies), each owner solves its range (bsdb_dev_gov_build_range, the
 * solve returning every key's rank) and writes its index slots [e_lo, e_lo +
 * n_g) at byte 8*e_lo of index.db (and index_a.db) in writes of <= 128 MiB.
 * Outputs the assembled structure in host arrays sized as bsdb_mph_export's:
 * h_E[num_buckets+1], h_values[bsdb_values_words(n)], h_sigbits[(n*width+63)/64
 * + 1] (NULL when width == 0) -- the fields of
 * GOVMinimalPerfectHashFunctionModified (GOV:284-313); bit-identical to the
 * one-device build, and the index files byte-identical.  index_path NULL: the
 * MPHF only (records ignored).  A device may be listed more than once (the
 * exchange is then a copy within it). */
int bsdb_multi_mph_build_index_fixed(bsdb_multi *mc, const uint8_t *h_keys, uint32_t key_len, uint64_t n,
                                     uint32_t width, const uint64_t *h_addr, const uint64_t *h_value8,
                                     const uint8_t *h_vlen, int approximate, const char *index_path,
                                     const char *index_a_path, uint64_t *h_E, uint64_t *h_values,
                                     uint64_t *h_sigbits);
int bsdb_multi_mph_build_index_var(bsdb_multi *mc, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n,
                                   uint32_t width, const uint64_t *h_addr, const uint64_t *h_value8,
                                   const uint8_t *h_vlen, int approximate, const char *index_path,
                                   const char *index_a_path, uint64_t *h_E, uint64_t *h_values, uint64_t *h_sigbits);

/* ---------------------------------------------------------------------------
 * A14/A15 + F1/F4 from host buffers: a GOV MPHF built on and resident on one
 * device (the Java side fills GOVMinimalPerfectHashFunctionModified's fields
 * from bsdb_mph_export and stores it with BinIO.storeObject, W:99-105;
 * INTEGRATION.md).  Keys as in bsdb_hash_*; seed 0 (CBHS:209).
 *   build     hash -> sort -> solve -> sign (width = hash.checksum.bits)
 *   info      n, num_buckets, width, words of the values / checksum arrays
 *   export    D2H: E[num_buckets+1] (offset | seed << 56), values words,
 *             checksum words (h_sigbits may be NULL when width == 0)
 *   import    H2D of the same arrays (e.g. from a loaded hash.db)
 *   dump/load the raw layout of GOV.dump (GOV:592-619) read by the
 *             reference's own load_mph (mph.c:28-43): native-endian u64
 *             n, multiplier, globalSeed, len(E), E[], len(array), array[];
 *             no checksum bits (load gives width 0)
 *   lookup    getLong (GOV:528-532, 557-569) of host keys: rank or -1
 *             (check != 0: range and checksum test; 0: unchecked rank)
 *   lifetime  an MPHF belongs to its context: bsdb_close releases the
 *             device arrays of the context's live MPHFs, after which their
 *             calls return BSDB_EINVAL and bsdb_mph_free only frees the
 *             handle (either order of bsdb_close / bsdb_mph_free is safe);
 *             close a bsdb_index before its MPHF
 * ------------------------------------------------------------------------- */
typedef struct bsdb_mph bsdb_mph;
int bsdb_mph_build_fixed(bsdb_ctx *ctx, const uint8_t *h_keys, uint32_t key_len, uint64_t n, uint32_t width,
                         bsdb_mph **out);
int bsdb_mph_build_var(bsdb_ctx *ctx, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n, uint32_t width,
                       bsdb_mph **out);
int bsdb_mph_info(const bsdb_mph *mph, uint64_t *n, uint64_t *num_buckets, uint32_t *width, uint64_t *values_words,
                  uint64_t *sig_words);
/* The sizes of an MPHF's fields on n keys with `width` checksum bits, without
 * a device or a handle (ABI 5; bsdb_mph_info returns the same numbers for a
 * built MPHF): num_buckets = n/1500 + 1 (GOV:350; E has num_buckets + 1
 * words, GOV:355); value_bits = 2 (1 + (n 281 >> 8)), the length of GOV's
 * 2-bit value vector with its trailing 0 (GOV:357,483-485), in values_words
 * u64 words; sig_words = ceil(n width / 64) + 1 words for the n width-bit
 * checksums (GOV:494; one zero word of slack), 0 when width == 0.  A JVM
 * sizes the arrays it exports into and wraps them with these
 * (LongArrayBitVector.wrap(values, value_bits)). */
int bsdb_mph_sizes(uint64_t n, uint32_t width, uint64_t *num_buckets, uint64_t *values_words, uint64_t *value_bits,
                   uint64_t *sig_words);
int bsdb_mph_export(bsdb_mph *mph, uint64_t *h_E, uint64_t *h_values, uint64_t *h_sigbits);
int bsdb_mph_import(bsdb_ctx *ctx, uint64_t n, uint32_t width, const uint64_t *h_E, const uint64_t *h_values,
                    const uint64_t *h_sigbits, bsdb_mph **out);
int bsdb_mph_dump(bsdb_mph *mph, const char *path);
int bsdb_mph_load(bsdb_ctx *ctx, const char *path, bsdb_mph **out);
int bsdb_mph_lookup_fixed(bsdb_mph *mph, const uint8_t *h_keys, uint32_t key_len, uint64_t n, int check,
                          int64_t *h_out);
int bsdb_mph_lookup_var(bsdb_mph *mph, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n, int check,
                        int64_t *h_out);
int bsdb_mph_free(bsdb_mph *mph);

/* ---------------------------------------------------------------------------
 * A13 + F2/F3: BSDBWriter.buildIndex (W:107-155, writeLBuffer W:166-179).
 * open: passSize = min(n, pass_cache_bytes / 8) slots, passes = ceil(n /
 *   passSize) (W:112-118); pass_cache_bytes == 0 sizes the pass cache by the
 *   device instead (a quarter of free HBM: one pass up to ~4 G records on an
 *   MI355X; the files are the same, only the number of kv.db scans changes).
 *   Creates/truncates index_path and index_a_path
 *   (the reference creates index_a.db even in exact mode, W:126; with
 *   index_a_path NULL it is not touched).  For each pass the caller feeds
 *   every record of the kv.db scan (KVWriter.forEach, W:134) with
 *   put_{var,fixed}: the key is looked up on the device (getLong, checked),
 *   and a record whose rank r lies in the pass writes the big-endian address
 *   (REVERSE_ORDER, Common.java:61) at slot r - rangeStart and, in approximate
 *   mode, the first min(len, 8) value bytes (value8 little-endian = the byte
 *   order in the record; a shorter value leaves its slot tail zero -- the
 *   reference leaves it unspecified, W:141).  end_pass writes the pass's slots
 *   in writes of <= 128 MiB.  Record buffers: key blob + offsets (or fixed
 *   keys), addr[count], and for approximate mode value8[count] + vlen[count]
 *   (min(value length, 8)).  Uploads are double-buffered on two streams.
 * ------------------------------------------------------------------------- */
typedef struct bsdb_index bsdb_index;

/* F2: the MPHF and index.db (+ index_a.db) in ONE call from
 * records in host memory -- hash -> GOV build whose solve also returns every
 * key's rank (the input position is carried through the bucket sort as the
 * store's payload, CBHS:386-388) -> addr[i] scattered big-endian at slot
 * rank[i] -> files in writes of <= 128 MiB.  No kv.db rescan and no lookup
 * pass: the files are identical to bsdb_index_* passes over the same
 * records (W:107-155).  The whole index lives on the device (8n B, 17n B more
 * in approximate mode); keys, addr[n], value8[n], vlen[n] as for put_*.
 * index_a_path may be NULL in exact mode (otherwise created empty, W:126). */
int bsdb_mph_build_index_fixed(bsdb_ctx *ctx, const uint8_t *h_keys, uint32_t key_len, uint64_t n, uint32_t width,
                               const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen,
                               int approximate, const char *index_path, const char *index_a_path, bsdb_mph **out);
int bsdb_mph_build_index_var(bsdb_ctx *ctx, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n, uint32_t width,
                             const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen, int approximate,
                             const char *index_path, const char *index_a_path, bsdb_mph **out);
/* F2 + F3 in bounded device memory: the same files and MPHF as
 * bsdb_mph_build_index_* from records in host memory, built by sequential
 * bucket-range passes over the keys kept in HBM (the reference's 256-segment
 * spill and segment-by-segment solve, CBHS:379-395,852-978, W:91-155): the
 * keys go to the device once, every pass re-hashes them and solves its range,
 * and each pass's index slots are written at their offset while the next pass
 * solves.  Reaches README-size sets on one device (C4: 13.19e9 x 13 B).
 * Addresses: h_addr[n], or (h_addr NULL) addr_base + addr_stride * i
 * (fixed-size records of one data file).  Addresses/values that do not fit
 * HBM beside the keys are gathered from the caller's arrays in host memory.
 * passes = 0 picks the fewest passes that fit; *passes_used (optional).
 * bsdb_mph_build_index_* take this path themselves when their one-shot build
 * does not fit the free HBM. */
int bsdb_mph_build_index_passes_fixed(bsdb_ctx *ctx, const uint8_t *h_keys, uint32_t key_len, uint64_t n,
                                      uint32_t width, const uint64_t *h_addr, uint64_t addr_base, uint64_t addr_stride,
                                      const uint64_t *h_value8, const uint8_t *h_vlen, int approximate, uint32_t passes,
                                      const char *index_path, const char *index_a_path, bsdb_mph **out,
                                      uint32_t *passes_used);
int bsdb_mph_build_index_passes_var(bsdb_ctx *ctx, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n,
                                    uint32_t width, const uint64_t *h_addr, uint64_t addr_base, uint64_t addr_stride,
                                    const uint64_t *h_value8, const uint8_t *h_vlen, int approximate, uint32_t passes,
                                    const char *index_path, const char *index_a_path, bsdb_mph **out,
                                    uint32_t *passes_used);

/* The same build fed incrementally, as BSDBWriter.put feeds the hash store
 * (W:75-89 -> CBHS:360-395): a builder owns the keys added so far in HBM (and,
 * unless addr_stride != 0 makes the address addr_base + addr_stride * (add
 * order), each record's address -- plus value8/vlen in approximate mode -- in
 * host memory).  key_len 0 = variable-length keys (add_fixed is accepted too);
 * key_capacity / blob_capacity reserve device memory up front (0 = grow on
 * demand).  Adds are synchronous (the caller may reuse its buffers) and may
 * come in any order: the files do not depend on it.  finish builds everything
 * added (index_path NULL: the MPHF only), releases the keys from HBM and
 * returns the MPHF; free releases the builder (after finish or instead of it).
 * A failed add leaves the builder failed (later calls return that code). */
typedef struct bsdb_builder bsdb_builder;
int bsdb_builder_open(bsdb_ctx *ctx, uint32_t key_len, uint64_t key_capacity, uint64_t blob_capacity, int approximate,
                      uint64_t addr_base, uint64_t addr_stride, bsdb_builder **out);
int bsdb_builder_add_fixed(bsdb_builder *b, const uint8_t *h_keys, uint32_t key_len, uint64_t count,
                           const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen);
int bsdb_builder_add_var(bsdb_builder *b, const uint8_t *h_blob, const uint64_t *h_off, uint64_t count,
                         const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen);
int bsdb_builder_count(const bsdb_builder *b, uint64_t *n);
int bsdb_builder_finish(bsdb_builder *b, uint32_t width, uint32_t passes, const char *index_path,
                        const char *index_a_path, bsdb_mph **out, uint32_t *passes_used);
int bsdb_builder_free(bsdb_builder *b);

int bsdb_index_open(bsdb_mph *mph, int approximate, uint64_t pass_cache_bytes, const char *index_path,
                    const char *index_a_path, bsdb_index **out, uint64_t *passes);
int bsdb_index_begin_pass(bsdb_index *ix, uint64_t pass);
int bsdb_index_put_var(bsdb_index *ix, const uint8_t *h_blob, const uint64_t *h_off, uint64_t count,
                       const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen);
int bsdb_index_put_fixed(bsdb_index *ix, const uint8_t *h_keys, uint32_t key_len, uint64_t count,
                         const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen);
int bsdb_index_end_pass(bsdb_index *ix);
int bsdb_index_close(bsdb_index *ix);

/* ---------------------------------------------------------------------------
 * F3: the kv.db scan that feeds buildIndex (W:134, PartitionedKVWriter.forEach
 * PKV:50-70), native: every partition file <kv_base>.<p> (PKV:79-81) is mapped
 * and parsed by a host thread into packed arrays in partition order -- the key
 * blob (+ offsets), each record's address as the reference computes it, the
 * first <= 8 value bytes (LE) and their count (index_a.db, W:140-142).
 * format 0 = SimpleCompactKVWriter (SimpleCompactKVWriter.java:55-70),
 * 1 = SimpleBlockedKVWriter with block_size-byte blocks (BlockedKVWriter.java:
 * 84-136).  threads <= 0: every hardware thread.  Host only (no device).
 * ------------------------------------------------------------------------- */
typedef struct bsdb_kv_records bsdb_kv_records;
int bsdb_kv_scan(const char *kv_base, int partitions, int format, uint32_t block_size, int threads,
                 bsdb_kv_records **out);
/* n records, their key bytes, and fixed_len = the common key length (0 when lengths differ) */
int bsdb_kv_records_info(const bsdb_kv_records *r, uint64_t *n, uint64_t *key_bytes, uint32_t *fixed_len);
/* borrowed pointers, valid until bsdb_kv_records_free: blob, offsets[n+1], addr[n], value8[n], vlen[n] */
int bsdb_kv_records_arrays(const bsdb_kv_records *r, const uint8_t **blob, const uint64_t **offsets,
                           const uint64_t **addr, const uint64_t **value8, const uint8_t **vlen);
int bsdb_kv_records_free(bsdb_kv_records *r);
/* W:91-155 straight from the data files: scan, then bsdb_mph_build_index_*
 * (hash, GOV build, ranks from the solve, index.db / index_a.db). */
int bsdb_kv_build_index(bsdb_ctx *ctx, const char *kv_base, int partitions, int format, uint32_t block_size,
                        int threads, uint32_t width, int approximate, const char *index_path,
                        const char *index_a_path, bsdb_mph **out);

/* ---------------------------------------------------------------------------
 * F4: the check of a finished database, batched on the device -- what
 * Builder -v does one synchronous lookup at a time (Builder.java:184-228:
 * getLong, the index.db slot, the kv.db record, a key compare).  Every record
 * goes key -> signature -> rank (checked getLong, GOV:557-569) -> slot in ONE
 * fused pass; a record passes when its key is accepted and the slot at its
 * rank holds the record's own big-endian address (and, index.approximate, the
 * first min(vlen, 8) bytes of its own value; the bytes past vlen are not
 * compared, W:141).  Record addresses are distinct by construction (partition
 * and file offset), so n passing records over an index.db of n slots occupy n
 * different ranks: the address test is the bijection test.
 *
 * The report is uint64_t out[BSDB_VERIFY_WORDS]:
 *   [0] records seen      [1] rejected (getLong gave -1)
 *   [2] in_window (accepted records whose rank lay in a window; every window
 *       together covers [0, n), so a clean run has [2] = [0] - [1])
 *   [3] wrong_addr        [4] wrong_value (counted independently of [3])
 *   [5] min_bad_addr: the smallest address among rejected / wrong_addr /
 *       wrong_value records (UINT64_MAX when none)
 *   [6] structure flags: bit 0 = E is not a valid offset array (E[0] = 0, low
 *       56 bits non-decreasing, E[m] = n; only a valid E keeps every lookup
 *       inside values[]: an imported hash.db is untrusted), bit 1 = index.db is
 *       not 8n bytes (or index_a.db, index.approximate), bit 2 = [0] != n
 *   [7] windows used
 * bsdb_dev_verify_*: records resident on the device (keys as in
 * bsdb_dev_hash_*: `count` of them, fixed-length keys at a 4-byte aligned
 * address; the address of record i is d_addr[i], or
 * addr_base + addr_stride * (first + i) when d_addr is NULL; d_value8 / d_vlen
 * as in bsdb_dev_index_scatter, read only with d_index_a) against the MPHF
 * arrays of bsdb_dev_lookup and the slots of the ranks [start, start + len) in
 * d_index (and d_index_a, 8-byte aligned, NULL in exact mode).  Asynchronous.
 * They ACCUMULATE into d_out[0..5] (the caller zeroes d_out and sets [5] to
 * all ones; several calls, e.g. one per key shard, add up) and set bit 0 of
 * d_out[6] when E is invalid, in which case no record is looked up.
 * bsdb_mph_verify_index_*: records in host memory as for bsdb_index_put_*,
 * the index files read from disk a window of ranks at a time (windows = 0: the
 * fewest windows whose slots fit half of the free HBM); with several windows
 * every window's pass sees all records: [0] and [1] come from the first pass,
 * [2..4] are summed, [5] is the minimum.  bsdb_kv_verify_index: the records
 * from the kv.db scan of bsdb_kv_build_index, each parsed chunk verified as it
 * arrives (host memory bounded as there; one rescan per window).
 * Returns: BSDB_EINVAL for bad arguments (before any device call),
 * BSDB_EFILE for a file that cannot be read, BSDB_EVERIFY with `out` filled
 * when any of [1], [3], [4], [6] is non-zero or [2] != [0] - [1], else BSDB_OK.
 * Flag bits 0 and 1 end the call before any record pass ([0] = 0).
 * ------------------------------------------------------------------------- */
#define BSDB_VERIFY_WORDS 8
int bsdb_dev_verify_fixed(bsdb_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint64_t count,
                          const uint64_t *d_addr, uint64_t addr_base, uint64_t addr_stride, uint64_t first,
                          const uint64_t *d_value8, const uint8_t *d_vlen, uint64_t n, uint64_t num_buckets,
                          const uint64_t *d_E, const uint64_t *d_values, uint32_t width, const uint64_t *d_sigbits,
                          uint64_t start, uint64_t len, const uint64_t *d_index, const uint8_t *d_index_a,
                          uint64_t *d_out, void *stream);
int bsdb_dev_verify_var(bsdb_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offsets,
                        uint64_t count, const uint64_t *d_addr, uint64_t addr_base, uint64_t addr_stride,
                        uint64_t first, const uint64_t *d_value8, const uint8_t *d_vlen, uint64_t n,
                        uint64_t num_buckets, const uint64_t *d_E, const uint64_t *d_values, uint32_t width,
                        const uint64_t *d_sigbits, uint64_t start, uint64_t len, const uint64_t *d_index,
                        const uint8_t *d_index_a, uint64_t *d_out, void *stream);
int bsdb_mph_verify_index_fixed(bsdb_mph *mph, const uint8_t *h_keys, uint32_t key_len, uint64_t count,
                                const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen,
                                int approximate, const char *index_path, const char *index_a_path, uint32_t windows,
                                uint64_t *out);
int bsdb_mph_verify_index_var(bsdb_mph *mph, const uint8_t *h_blob, const uint64_t *h_off, uint64_t count,
                              const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen,
                              int approximate, const char *index_path, const char *index_a_path, uint32_t windows,
                              uint64_t *out);
int bsdb_kv_verify_index(bsdb_mph *mph, const char *kv_base, int partitions, int format, uint32_t block_size,
                         int threads, int approximate, const char *index_path, const char *index_a_path,
                         uint32_t windows, uint64_t *out);

/* ---------------------------------------------------------------------------
 * Which keys are duplicates: the query behind BSDB_EDUP.  "Keys must not have
 * duplicates" is the reference's one hard input rule (CBHS:969-972,
 * GOV:471-479); a build that meets two equal 128-bit signatures returns
 * BSDB_EDUP and no more.  These calls run the build's grouping again (hash,
 * bucket, sort with each key's input position, by bucket-range passes; no
 * solve) and list the colliding records.  They change nothing in the build:
 * BSDB_EDUP is returned where it always was.
 *
 * Groups and pairs.  A group is a maximal set of input keys with equal
 * (sig0, sig1) at seed 0, as the build hashes them.  A group of r keys is
 * reported as r - 1 pairs (anchor, other); in the device and host forms
 * anchor is the group's smallest input position.  The list is in no
 * particular order.  Each pair has a kind byte:
 *   BSDB_DUP_SAME_KEY    the two keys' bytes and lengths are equal
 *   BSDB_DUP_COLLISION   they differ: distinct keys with one signature (the
 *                        reference reseeds then; this build cannot)
 *   BSDB_DUP_UNCOMPARED  the key bytes were not available (a builder in spill
 *                        mode keeps signatures and positions only)
 * The report is uint64_t[BSDB_DUP_WORDS]:
 *   [0] pairs found: the total, which may exceed cap
 *   [1] how many of the LISTED pairs are BSDB_DUP_COLLISION
 *   [2] flags: BSDB_DUP_LIST_FULL = found > cap (the list then holds some cap
 *       of the pairs, all valid and distinct); BSDB_DUP_PARTIAL = a bucket held
 *       more than 16 384 keys (the sort's limit, where the build returns
 *       BSDB_E2BIG): its keys were examined in consecutive chunks of 16 384,
 *       so a group may be reported as one group per chunk, a key with a single
 *       copy in each of two chunks is missed, and [0] is a lower bound --
 *       remove what was reported and run again
 *   [3] keys examined
 * Finding duplicates is not an error: every form returns BSDB_OK with
 * [0] >= 0; the usual codes report bad arguments, memory and I/O.  cap = 0
 * (no list, d_pairs / d_kinds may be NULL) still counts.  All forms return
 * after the device finished.  Device memory per pass: 16 + 8 B per key of the
 * pass, plus the list (16 + 1 B per pair of cap).
 *
 * bsdb_dev_find_duplicates_fixed / _var: keys resident on the device, as for
 *   bsdb_dev_mph_build_index_passes_* (d_keys / d_blob 4-byte aligned);
 *   passes = 0 picks the fewest passes that fit the free HBM.  d_pairs[2 cap]
 *   (u64 positions), d_kinds[cap] (may be NULL: not compared),
 *   d_report[BSDB_DUP_WORDS].
 * bsdb_dev_find_duplicates_sig: n signatures (sig0, sig1 interleaved, 16-byte
 *   aligned) in one pass; positions are indices into d_sig; no kinds.  A rank
 *   of a sharded (E4) build can call it on the signatures it owns (buckets
 *   are those of its own n, so a narrow sig0 range only sorts larger buckets).
 * bsdb_dev_classify_pairs_fixed / _var: d_kinds[i] = BSDB_DUP_SAME_KEY or
 *   BSDB_DUP_COLLISION for the keys at positions d_pairs[2i], d_pairs[2i+1] of
 *   the n keys (a position >= n gives BSDB_DUP_COLLISION); d_keys 4-byte
 *   aligned, d_blob at any address.  Asynchronous.  The
 *   key forms call it on their own list; it is exported because a signature
 *   collision of distinct keys cannot be provoked through real hashing.
 * bsdb_find_duplicates_fixed / _var: keys in host memory, streamed through a
 *   builder (device memory bounded as for the build; past the device's key
 *   area the builder spills and every kind is BSDB_DUP_UNCOMPARED).
 * bsdb_builder_find_duplicates: everything added so far, valid before
 *   bsdb_builder_finish (BSDB_EINVAL after it, as a second finish).  Reports
 *   record ADDRESSES, not positions -- the caller's h_addr, or addr_base +
 *   addr_stride * position -- which a caller that adds from several threads
 *   can map back; which member of a group is the anchor is unspecified.
 * bsdb_kv_find_duplicates: the kv.db scan of bsdb_kv_build_index into a
 *   builder, then the builder form: what a caller runs after
 *   bsdb_kv_build_index returned BSDB_EDUP.  Addresses as bsdb_kv_scan's.
 * ------------------------------------------------------------------------- */
#define BSDB_DUP_WORDS 4
#define BSDB_DUP_SAME_KEY 0
#define BSDB_DUP_COLLISION 1
#define BSDB_DUP_UNCOMPARED 2
#define BSDB_DUP_LIST_FULL 1
#define BSDB_DUP_PARTIAL 2
int bsdb_dev_find_duplicates_fixed(bsdb_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint64_t n, uint32_t passes,
                                   uint64_t cap, uint64_t *d_pairs, uint8_t *d_kinds, uint64_t *d_report, void *stream);
int bsdb_dev_find_duplicates_var(bsdb_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off,
                                 uint64_t n, uint32_t passes, uint64_t cap, uint64_t *d_pairs, uint8_t *d_kinds,
                                 uint64_t *d_report, void *stream);
int bsdb_dev_find_duplicates_sig(bsdb_ctx *ctx, const uint64_t *d_sig, uint64_t n, uint64_t cap, uint64_t *d_pairs,
                                 uint64_t *d_report, void *stream);
int bsdb_dev_classify_pairs_fixed(bsdb_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint64_t n,
                                  const uint64_t *d_pairs, uint64_t count, uint8_t *d_kinds, void *stream);
int bsdb_dev_classify_pairs_var(bsdb_ctx *ctx, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off,
                                uint64_t n, const uint64_t *d_pairs, uint64_t count, uint8_t *d_kinds, void *stream);
int bsdb_find_duplicates_fixed(bsdb_ctx *ctx, const uint8_t *h_keys, uint32_t key_len, uint64_t n, uint64_t cap,
                               uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report);
int bsdb_find_duplicates_var(bsdb_ctx *ctx, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n, uint64_t cap,
                             uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report);
int bsdb_builder_find_duplicates(bsdb_builder *b, uint64_t cap, uint64_t *h_addr_pairs, uint8_t *h_kinds,
                                 uint64_t *report);
int bsdb_kv_find_duplicates(bsdb_ctx *ctx, const char *kv_base, int partitions, int format, uint32_t block_size,
                            int threads, uint64_t cap, uint64_t *h_addr_pairs, uint8_t *h_kinds, uint64_t *report);

/* ---------------------------------------------------------------------------
 * Batched get: a finished database read on the device, key -> value.  What
 * SyncReader.getAsBytes does one key per call (read/SyncReader.java:44-57 ->
 * BaseKVReader.getValueAsBytes, read/kv/BaseKVReader.java:16-31), for a batch:
 * key -> signature -> rank (checked getLong, GOV:557-569) -> index.db slot ->
 * address -> record -> key compare -> the value bytes, packed.
 *
 * bsdb_db_open makes the database resident.  format / block_size as for
 * bsdb_kv_scan (0 compact, 1 blocked).  Exact mode (approximate = 0): index_path
 * is index.db, loaded whole (it must be 8n bytes: BSDB_EVERIFY otherwise, as
 * flag bit 1 of the verify report), and every <kv_base>.<p>, p < partitions
 * <= 128 (an address is non-negative: 7 partition bits), is loaded into ONE
 * device allocation, each partition at a 16-byte aligned base.  Approximate
 * mode: index_path is index_a.db (8n bytes), no kv.db is read and kv_base may
 * be NULL.  E is validated before any lookup is allowed, as the verify calls
 * do (an imported hash.dump is untrusted: BSDB_EVERIFY when E is no valid
 * offset array).  BSDB_ENOMEM when the files do not fit the free device
 * memory: a host-resident or windowed kv.db is out of scope, and so are
 * compressed kv.db files.  The db borrows the MPHF, as a bsdb_index does:
 * after bsdb_mph_free or bsdb_close its calls return BSDB_EINVAL and
 * bsdb_db_free only releases it (any order is safe).
 * bsdb_db_info fills uint64_t[BSDB_DB_INFO_WORDS]: n, partitions, format,
 * block_size, approximate, image bytes, index bytes, host chunk (queries).
 *
 * Every query gets a status byte, tested in this order:
 *   BSDB_GET_REJECTED      getLong gave -1 (rank >= n, or the checksum bits differ)
 *   BSDB_GET_BAD_ADDR      the slot's address does not denote a whole record
 *                          inside the resident files: top bit set (SyncReader.java:
 *                          52 returns null), partition >= partitions
 *                          (PartitionedKVReader.java:78-82: partition = addr >>> 56,
 *                          offset = low 56 bits), blocked layout
 *                          (BlockedKVReader.java:42-52: block offset = ((addr >>>
 *                          16) & 0xFFFFFFFF) * 4096, block size = ((addr >>> 48) &
 *                          0xFF) * 4096, record offset = addr & 0xFFFF) with a
 *                          block of size 0 or not inside its file, or the record
 *                          [pos, pos + 3 + kLen + vLen) ([kLen u8][vLen u16 BE]
 *                          [key][value]) not inside its file (compact) or its
 *                          block (blocked).  index.db is untrusted: no byte
 *                          outside the resident files is ever read.
 *   BSDB_GET_KEY_MISMATCH  the record holds another key (kLen or bytes differ:
 *                          the reference returns null, BaseKVReader.java:65-83)
 *   BSDB_GET_FOUND         the value is returned
 * A query that is not FOUND has value length 0.  Approximate mode has only
 * FOUND and REJECTED: a found value is the 8 raw bytes of the slot
 * (LBufferIndexReader.getRawBytesAt), no key compare, false positives included.
 *
 * The report is uint64_t[BSDB_GET_WORDS]:
 *   [0] queries           [1] found
 *   [2] rejected          [3] key_mismatch
 *   [4] bad_addr          [5] value_bytes (the sum over found queries)
 * bsdb_dev_db_locate_*: keys resident on the device as for bsdb_dev_verify_*
 *   (fixed-length keys at a 4-byte aligned address).  Writes per query d_src
 *   (the byte position of the value in the device image; approximate mode: the
 *   slot), d_vlen (u32) and d_status, and ACCUMULATES into d_report (zeroed by
 *   the caller, 8-byte aligned).  Asynchronous.
 * The offsets are the u32 -> u64 exclusive scan of d_vlen, nq + 1 entries:
 *   bsdb_dev_edge_offsets(ctx, d_vlen, nq, d_voff, stream).
 * bsdb_dev_db_gather: value i to d_values[d_voff[i] .. d_voff[i + 1]);
 *   value_bytes = d_voff[nq].  d_values may start at any address; nothing is
 *   written outside [d_values, d_values + value_bytes).  Asynchronous.
 * bsdb_db_get_*: keys in host memory (as bsdb_hash_*), streamed in chunks of
 *   bsdb_db_set_batch queries (0 = default).  h_voff[nq + 1] is the exclusive
 *   prefix of the value lengths over the whole call, h_voff[nq] = report[5];
 *   value i is h_values[h_voff[i] .. h_voff[i + 1]).  When report[5] >
 *   value_cap the call returns BSDB_E2BIG with h_voff, h_status and report
 *   complete and h_values unspecified: the caller retries with report[5].
 *   nq = 0 is BSDB_OK with h_voff[0] = 0.
 * Returns: BSDB_EINVAL for bad arguments (before any device call), BSDB_EFILE
 * for a file that cannot be read, else as above.
 * ------------------------------------------------------------------------- */
typedef struct bsdb_db bsdb_db;
#define BSDB_DB_INFO_WORDS 8
#define BSDB_GET_WORDS 6
#define BSDB_GET_FOUND 0
#define BSDB_GET_REJECTED 1
#define BSDB_GET_KEY_MISMATCH 2
#define BSDB_GET_BAD_ADDR 3
int bsdb_db_open(bsdb_mph *mph, const char *kv_base, int partitions, int format, uint32_t block_size, int approximate,
                 const char *index_path, bsdb_db **out);
int bsdb_db_info(const bsdb_db *db, uint64_t *out /* BSDB_DB_INFO_WORDS */);
int bsdb_db_set_batch(bsdb_db *db, uint64_t max_queries);
int bsdb_db_get_fixed(bsdb_db *db, const uint8_t *h_keys, uint32_t key_len, uint64_t nq, uint64_t value_cap,
                      uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status, uint64_t *report);
int bsdb_db_get_var(bsdb_db *db, const uint8_t *h_blob, const uint64_t *h_off, uint64_t nq, uint64_t value_cap,
                    uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status, uint64_t *report);
int bsdb_db_free(bsdb_db *db);
int bsdb_dev_db_locate_fixed(bsdb_db *db, const uint8_t *d_keys, uint32_t key_len, uint64_t nq, uint64_t *d_src,
                             uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream);
int bsdb_dev_db_locate_var(bsdb_db *db, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off, uint64_t nq,
                           uint64_t *d_src, uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream);
int bsdb_dev_db_gather(bsdb_db *db, const uint64_t *d_src, const uint64_t *d_voff, uint64_t nq, uint8_t *d_values,
                       uint64_t value_bytes, void *stream);

/* ---- text front end: "key<sep>value" lines -> records -> kv.db + database ----
 * What tools/Builder.java:144-176 does one line per call on one thread per
 * input file: split text into lines and fields, keep the lines that are
 * records, write them in the compact kv.db layout ([kLen u8][vLen u16 BE][key]
 * [value], SimpleCompactKVWriter.java:36-42) and hand their keys to the build.
 *
 * The record rule (BufferedReader.lines, String.split(sep), Builder.java:148-160):
 *   lines    a line ends at "\n", at "\r" or at "\r\n"; a last line without a
 *            terminator is a line; nothing follows the final terminator (the
 *            empty text has 0 lines, "\n" one empty line).  Byte i starts a line
 *            iff i == 0, or t[i-1] == '\n', or (t[i-1] == '\r' and t[i] != '\n').
 *   fields   the line is split at every separator byte and trailing empty
 *            fields are dropped; it is a record iff exactly two fields remain:
 *            key = field 0, value = field 1.  Everything else counts as
 *            not_two_fields.
 *   then     a key of 0 bytes is dropped (empty_key; a DEVIATION: the reference
 *            would put it, this library's writers take keys of 1..255 bytes);
 *            a key over 255 or a value over 32 510 bytes (Common.MAX_VALUE_SIZE)
 *            is dropped (too_large).
 *   bytes    taken verbatim: bytes >= 0x80 and NUL are data.  Malformed UTF-8,
 *            which Java's decoder would replace, is out of scope (a DEVIATION
 *            for such input only).  The separator is ONE literal byte < 0x80
 *            that is neither '\r' nor '\n' (else BSDB_EINVAL); a byte that
 *            String.split would read as a regex meta-character ('|', '.', '*'
 *            ...) is taken literally here (a DEVIATION).
 *   order    kept records keep input order: files in the order given, then
 *            lines in file order.
 * The report is uint64_t[BSDB_TEXT_WORDS], ACCUMULATED by the dev_ call:
 *   [0] lines  [1] records  [2] not_two_fields  [3] empty_key  [4] too_large
 *   [5] key_bytes  [6] value_bytes  [7] max_key_len  [8] max_value_len
 *   [9] chunks;   lines == records + not_two_fields + empty_key + too_large.
 *
 * bsdb_text_max_records: the most records `bytes` of text can hold,
 *   bytes / 4 + 1 (host only).
 * bsdb_dev_text_split: d_text (16-byte aligned, bytes < 2^32) on the device
 *   -> the kept records' descriptors in input order: key at d_text[d_kpos[r]
 *   .. + d_klen[r]), value at d_text[d_vpos[r] .. + d_vlen[r]); capacity >=
 *   bsdb_text_max_records(bytes) entries each, else BSDB_EINVAL.  d_report
 *   (8-byte aligned, zeroed by the caller) accumulates; [1] tells how many
 *   descriptors were written.  Enqueued on `stream`; the call waits once for
 *   the count kernel (the numbers of lines and separators size its
 *   workspace), the rest is asynchronous.
 * bsdb_dev_text_pack: `count` descriptors of that text -> the chunk's image,
 *   the records back to back, cut by the PARTITION RULE into `partitions`
 *   (1..128) contiguous runs, run p = records [p count / P, (p + 1) count / P)
 *   (the reference leaves the assignment open, PartitionedKVWriter.java:82-96):
 *   run p is to be appended to kv.db.<p> at h_part_size[p], its bytes come back
 *   in h_run_bytes[p] (the runs lie in d_image in order, so they leave as P
 *   plain copies); d_addr[r] = p << 56 | file offset of record r; d_blob /
 *   d_off[count + 1] the packed keys with their offsets from 0 (*h_blob_bytes =
 *   d_off[count]); d_value8 / d_value_len (both or neither) the index_a.db
 *   payload: the first min(vLen, 8) value bytes, the rest 0, and that length.
 *   d_image, d_blob and d_value_len may start at any address; nothing is written
 *   outside the bytes reported.  BSDB_EINVAL when image_cap or blob_cap is too
 *   small (nothing written; 1.5 x bytes + 16 and bytes + 16 always suffice) or
 *   a file would pass 2^56 bytes.  The call returns with the sizes, so it waits
 *   for its scans; the pack kernels are left running on `stream`.
 * bsdb_builder_add_dev_var: bsdb_builder_add_var with the batch in device
 *   memory (d_off[0 .. count] into d_blob, the record arrays as for the host
 *   add).  The keys and offsets are copied device to device, the record arrays
 *   to the builder's host arrays (and device arrays, when it keeps them); a
 *   builder in spill mode takes the batch through host memory and the host add.
 *   The caller's buffers are free when the call returns.  Builders of
 *   variable-length keys only.
 * bsdb_text_set_chunk: text bytes bsdb_text_build handles at a time (0 =
 *   default 256 MiB; at least 64 KiB; capped so that a chunk's device footprint
 *   fits half of the free device memory).
 * bsdb_text_build: Builder's put loop and build(): every file of paths[0 ..
 *   nfiles) is read a chunk at a time, cut after the chunk's last line end (the
 *   rest is carried to the next chunk; chunks never span files, and a file's
 *   unterminated last line does not join the next file), split, packed, its
 *   runs appended to kv_base.<p> (created or truncated) and its keys added to a
 *   streaming builder on the device; the finish writes index_path /
 *   index_a_path as bsdb_builder_finish does.  `report` (host) is the whole
 *   input's.  A line longer than the chunk returns BSDB_E2BIG (a DEVIATION: Java
 *   takes lines of any length).  BSDB_EDUP comes back as from any build: the
 *   kv.db files are complete then, so bsdb_kv_find_duplicates names the records.
 *   The empty input builds the empty database.
 *
 * THE BLOCKED LAYOUT (format 1; what the reference's Builder writes without
 * -c: SimpleBlockedKVWriter with 4096-byte blocks, BlockedKVWriter.java:45-74,
 * :134-136).  The placement rule, for one run (the records the partition rule
 * gives partition p in one chunk, in input order), a block size B and the size
 * F of kv.db.<p> before the run; size = 3 + kLen + vLen:
 *   small    (size <= B)  if a block is open and B - fill < size, the open block
 *            is closed: appended to the file at its current end.  The record's
 *            offset in the (then open, or newly opened) block is fill; fill +=
 *            size.  A record that exactly fills the block leaves it open and
 *            full; the next small record closes it.
 *   large    (size > B; text records are at most 32 768 bytes, so only for B <
 *            32 768)  a block of its own of ceil(size / 4096) x 4096 bytes, at
 *            offset 0, appended AT ONCE, ahead of the block that is open at that
 *            moment; that block stays open and keeps filling.
 *   end      the run's end closes the open block.  DEVIATION 6: the reference's
 *            open block lives on across puts until finish; here every chunk's
 *            run ends its block, at most one partial block per partition and
 *            chunk.  The reference's reader and scan step over such a block like
 *            any other (BlockedKVWriter.java:90-117).
 *   bytes    a block's records sit back to back from offset 0, every other byte
 *            of the block is 0, the end mark after the last record included; a
 *            record's first byte (kLen >= 1) is never 0.
 *   address  p << 56 | (block bytes / 4096) << 48 | (block file position / 4096)
 *            << 16 | offset.
 *   limits   B a multiple of 4096 in 4096 .. 65 536 (16 bits of offset); F a
 *            multiple of 4096; no file beyond 2^44 bytes (32 bits of pages);
 *            else BSDB_EINVAL.
 * bsdb_text_image_max: an upper bound of a chunk's image (host only): format 0
 *   1.5 x bytes + 16; format 1 2 x (bytes + bytes / 4 + 2) + partitions x
 *   block_size + 16.
 * bsdb_dev_text_pack_blocked: bsdb_dev_text_pack into the blocked layout.
 *   h_part_size[p] must be a multiple of 4096; h_run_bytes[p] comes back as one:
 *   run p's image is its file bytes in file order, the runs back to back in
 *   d_image.  The key blob, its offsets and the value heads are those of
 *   bsdb_dev_text_pack.  BSDB_EINVAL, with nothing written, when image_cap or
 *   blob_cap is too small or an argument breaks the limits.
 * bsdb_text_build_layout: bsdb_text_build with the layout chosen: format 0
 *   (block_size ignored) is bsdb_text_build itself, format 1 writes blocked
 *   kv.db files that bsdb_kv_scan / bsdb_kv_verify_index / bsdb_db_open read
 *   with format = 1 and the same block_size.
 * ------------------------------------------------------------------------- */
#define BSDB_TEXT_WORDS 10
uint64_t bsdb_text_max_records(uint64_t bytes);
int bsdb_dev_text_split(bsdb_ctx *ctx, const uint8_t *d_text, uint64_t bytes, int separator, uint64_t capacity,
                        uint32_t *d_kpos, uint32_t *d_klen, uint32_t *d_vpos, uint32_t *d_vlen, uint64_t *d_report,
                        void *stream);
int bsdb_dev_text_pack(bsdb_ctx *ctx, const uint8_t *d_text, uint64_t bytes, const uint32_t *d_kpos,
                       const uint32_t *d_klen, const uint32_t *d_vpos, const uint32_t *d_vlen, uint64_t count,
                       int partitions, const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap,
                       uint64_t *h_run_bytes, uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off,
                       uint64_t *h_blob_bytes, uint64_t *d_value8, uint8_t *d_value_len, void *stream);
int bsdb_builder_add_dev_var(bsdb_builder *b, const uint8_t *d_blob, const uint64_t *d_off, uint64_t count,
                             const uint64_t *d_addr, const uint64_t *d_value8, const uint8_t *d_vlen, void *stream);
int bsdb_text_set_chunk(bsdb_ctx *ctx, uint64_t bytes);
int bsdb_text_build(bsdb_ctx *ctx, const char *const *paths, int nfiles, int separator, const char *kv_base,
                    int partitions, uint32_t width, int approximate, const char *index_path, const char *index_a_path,
                    uint64_t *report /* BSDB_TEXT_WORDS */, bsdb_mph **out);
uint64_t bsdb_text_image_max(uint64_t bytes, int partitions, int format, uint32_t block_size);
int bsdb_dev_text_pack_blocked(bsdb_ctx *ctx, const uint8_t *d_text, uint64_t bytes, const uint32_t *d_kpos,
                               const uint32_t *d_klen, const uint32_t *d_vpos, const uint32_t *d_vlen, uint64_t count,
                               int partitions, uint32_t block_size, const uint64_t *h_part_size, uint8_t *d_image,
                               uint64_t image_cap, uint64_t *h_run_bytes, uint64_t *d_addr, uint8_t *d_blob,
                               uint64_t blob_cap, uint64_t *d_off, uint64_t *h_blob_bytes, uint64_t *d_value8,
                               uint8_t *d_value_len, void *stream);
int bsdb_text_build_layout(bsdb_ctx *ctx, const char *const *paths, int nfiles, int separator, const char *kv_base,
                           int partitions, int format, uint32_t block_size, uint32_t width, int approximate,
                           const char *index_path, const char *index_a_path, uint64_t *report /* BSDB_TEXT_WORDS */,
                           bsdb_mph **out);

/* ---- a database checked against text input: key -> value compare ------------
 * What the reference's Builder does with -v (tools/Builder.java:184-228): the
 * input is read a second time, getAsBytes(key) is called for every record and
 * the bytes it returns are compared with the value in the text.  Here, for a
 * chunk of text on the device: the split gives the records, bsdb_dev_db_locate_var
 * gives, per key, where the resident database's value lies, and the check
 * compares the text's value bytes with the image's in place.  No value is
 * gathered or written.  (bsdb_kv_verify_index walks the kv.db files and never
 * reads the text: a record the split dropped, or a value taken from the wrong
 * line, passes it.)
 *
 * Every record gets a status byte; the get's codes are kept:
 *   0 OK                      found, the same length, the same bytes
 *   1 BSDB_GET_REJECTED, 2 BSDB_GET_KEY_MISMATCH, 3 BSDB_GET_BAD_ADDR   as for the get
 *   4 BSDB_CHECK_VALUE_LEN    found, the database's value has another length
 *   5 BSDB_CHECK_VALUE_BYTES  found, the same length, some byte differs
 * Approximate mode (the db holds index_a.db): the slot's 8 bytes are compared
 * with the value head the text front end stores for the text's value (its first
 * min(vLen, 8) bytes, the rest 0); there is no length status, and the false
 * positive of an absent key shows up as VALUE_BYTES (or, when the slot happens
 * to hold the same head, as OK).
 * The report is uint64_t[BSDB_CHECK_WORDS], ACCUMULATED by the dev_ call:
 *   [0] records   [1] ok   [2] rejected   [3] key_mismatch   [4] bad_addr
 *   [5] value_len   [6] value_bytes
 *   [7] first_bad: the smallest input-order index of a record that is not OK,
 *       UINT64_MAX when there is none;   [0] == [1] + ... + [6].
 *
 * bsdb_dev_db_check: d_text (16-byte aligned, text_bytes < 2^32) is the chunk,
 *   d_vpos / d_vlen the `count` kept records' value descriptors from
 *   bsdb_dev_text_split, d_src / d_dbvlen / d_status what bsdb_dev_db_locate_var
 *   returned for their keys (the key blob: bsdb_dev_text_pack).  d_status comes
 *   in as locate's and goes out as the check's (a byte that is none of the get's
 *   codes counts as BAD_ADDR).  d_report (8-byte aligned) is zeroed by the caller
 *   with [7] = UINT64_MAX, and accumulates; record_base is the input-order index
 *   of record 0, so [7] is global over the caller's chunks.  Descriptors,
 *   positions and lengths are data: no byte outside the text and the image is
 *   read, and a database length over 65 535 (none a record can have) is
 *   VALUE_LEN.  The workspace is the context's.  Asynchronous.  BSDB_EINVAL before
 *   any device call for null or misaligned arguments or text_bytes >= 2^32.
 * bsdb_db_check_text: every file of paths[0 .. nfiles) is read a chunk at a
 *   time exactly as bsdb_text_build reads it (the same cut rule, and
 *   bsdb_text_set_chunk of the db's context; the chunk is halved until its
 *   footprint fits half of the device memory that is free beside the resident
 *   database), split, its keys packed, located and checked.  text_report is the
 *   split's (BSDB_TEXT_WORDS), check_report the check's.  The records that are
 *   not OK are appended in input order to h_bad_file (the index into paths),
 *   h_bad_offset (the file offset of the first byte of the record's key) and
 *   h_bad_status until bad_cap entries are held; *n_bad counts all of them.
 *   Returns BSDB_OK when every record is OK, BSDB_EVERIFY with all outputs filled
 *   when one is not, BSDB_E2BIG for a line longer than a chunk, BSDB_EFILE for a
 *   file that cannot be read, BSDB_EINVAL for bad arguments (before any device
 *   call) or a db whose MPHF was freed.  The empty input is BSDB_OK with all
 *   counts 0.  It tells whether every record of the text is in the database, not
 *   the converse: compare [1] with bsdb_db_info's n for that.
 * Out of scope: compressed kv.db, a database that does not fit the device beside
 * a chunk of text, overlapping the file reads with the device work.
 * ------------------------------------------------------------------------- */
#define BSDB_CHECK_WORDS 8
#define BSDB_CHECK_VALUE_LEN 4
#define BSDB_CHECK_VALUE_BYTES 5
int bsdb_dev_db_check(bsdb_db *db, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_vpos,
                      const uint32_t *d_vlen, const uint64_t *d_src, const uint32_t *d_dbvlen, uint8_t *d_status,
                      uint64_t count, uint64_t record_base, uint64_t *d_report, void *stream);
int bsdb_db_check_text(bsdb_db *db, const char *const *paths, int nfiles, int separator,
                       uint64_t *text_report /* BSDB_TEXT_WORDS */, uint64_t *check_report /* BSDB_CHECK_WORDS */,
                       uint64_t bad_cap, uint32_t *h_bad_file, uint64_t *h_bad_offset, uint8_t *h_bad_status,
                       uint64_t *n_bad);

/* ---- a resident database enumerated by slot: records, items, a text dump ----
 * index.db is n slots and every slot is the address of one record, so a
 * resident database lists itself: slot r (the rank the MPHF gives r's key) ->
 * address -> 3-byte header -> key and value.  No key is needed, nothing is
 * hashed.  The order is slot order, rank 0 .. n - 1: deterministic for a given
 * database, and any window [first, first + count) can be taken on its own.
 * (The reference has no dump; KVWriter.forEach walks the files in file order
 * for buildIndex.)  Exact mode only: an approximate database holds no records,
 * and every call here returns BSDB_EINVAL for it.
 *
 * Every slot gets a status byte:
 *   BSDB_SCAN_OK        the slot names a whole record
 *   BSDB_SCAN_BAD_ADDR  its address does not (the rule of BSDB_GET_BAD_ADDR,
 *                       the same function); both lengths and positions are 0,
 *                       and it writes nothing to a text
 *   BSDB_SCAN_NOT_TEXT  set only by the text calls: the record's line
 *                       key<sep>value\n does not read back as that record
 *                       through the text front end (bsdb_text_build): the key
 *                       or the value is empty, the value is longer than
 *                       32 510 bytes, or a key or value byte is the separator,
 *                       0x0A or 0x0D.  Its bytes are written raw all the same;
 *                       the report says the text cannot carry them, and the
 *                       caller decides.
 * The report is uint64_t[BSDB_SCAN_WORDS], ACCUMULATED by the dev_ calls into
 * words the caller zeroed, with [7] = UINT64_MAX:
 *   [0] slots   [1] ok   [2] bad_addr   [3] not_text   [0] == [1] + [2] + [3]
 *   [4] key_bytes   [5] value_bytes   (of the slots that are not BAD_ADDR)
 *   [6] text_bytes  (0 from bsdb_dev_db_records and bsdb_db_scan)
 *   [7] first_bad: the lowest slot that is not OK, UINT64_MAX when there is none
 * bsdb_dev_db_records and bsdb_dev_db_dump_text each fill a whole report for
 * the records they see: give each its own, or the counts add up twice.
 *
 * bsdb_dev_db_records: for slot first + i, i < count: d_ksrc[i] / d_vsrc[i]
 *   (u64, 8-byte aligned) the byte positions of key and value in the resident
 *   image, d_klen[i] / d_vlen[i] (u32, so bsdb_dev_edge_offsets scans them),
 *   d_status[i].  Packed keys and values need no further call of their own:
 *   bsdb_dev_edge_offsets over d_klen (d_vlen), then bsdb_dev_db_gather with
 *   d_ksrc (d_vsrc).  Asynchronous.
 * bsdb_dev_db_dump_lengths: d_llen[i] = the bytes of record i's line (kLen + 1
 *   + vLen + 1, 0 for BAD_ADDR), d_loff[count + 1] their exclusive scan;
 *   d_status comes in as bsdb_dev_db_records' and goes out with the length
 *   part of NOT_TEXT (a byte that is none of the codes counts as BAD_ADDR).
 *   The caller reads d_loff[count], the text's length, before the next call
 *   (as the get leaves its scan to the caller).  The workspace is the
 *   context's.  Asynchronous.
 * bsdb_dev_db_dump_text: the text_bytes = d_loff[count] bytes of the lines to
 *   d_text (any alignment), the bytes' part of NOT_TEXT into d_status, then the
 *   report; `first` is the slot of record 0, so [7] is a slot.  Descriptors and
 *   offsets are data: no byte outside the image is read (a position past it
 *   reads as 0), lengths are cut to what a header holds (255, 65 535), offsets
 *   that are no scan leave zeros, and nothing is written outside [d_text,
 *   d_text + text_bytes).  Asynchronous.
 * bsdb_db_scan: the window's records in host memory, streamed in chunks of
 *   bsdb_db_set_batch slots: h_keys / h_koff[count + 1] and h_values /
 *   h_voff[count + 1] packed with offsets over the whole call, h_status[count].
 *   Past key_cap or value_cap it goes on without gathering that side and
 *   returns BSDB_E2BIG with offsets, status and report complete (report [4],
 *   [5] are the sizes to come back with), as bsdb_db_get_* does.
 * bsdb_db_dump_text: the window's lines to the file `path` (created;
 *   truncated unless `append`), a chunk of slots at a time, each cut so that
 *   its text stays under the cap of bsdb_db_set_text_chunk (0 = the default,
 *   256 MiB; a cap below the longest line, 255 + 65 535 + 2 bytes, is
 *   BSDB_EINVAL): never more than one such piece of text is held on either
 *   side.  Returns BSDB_OK whatever the statuses: report [2], [3] and [7] say
 *   whether the text carries the database.
 * All: BSDB_EINVAL before any device call for null or misaligned arguments, a
 *   bad separator (as for bsdb_text_build), first + count > n, an approximate
 *   db or one whose MPHF was freed; count == 0 is BSDB_OK with an empty result;
 *   BSDB_EFILE for a file that cannot be written.
 * The diff of two databases is the next block's (bsdb_db_diff).
 * Out of scope: escaping NOT_TEXT records, other line terminators, compressed
 * kv.db, a kv.db larger than device memory, and whether each slot is its own key's (bsdb_kv_verify_index: a dump presumes a
 * verified database).
 * ------------------------------------------------------------------------- */
#define BSDB_SCAN_WORDS 8
#define BSDB_SCAN_OK 0
#define BSDB_SCAN_BAD_ADDR 1
#define BSDB_SCAN_NOT_TEXT 2
int bsdb_dev_db_records(bsdb_db *db, uint64_t first, uint64_t count, uint64_t *d_ksrc, uint32_t *d_klen,
                        uint64_t *d_vsrc, uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream);
int bsdb_dev_db_dump_lengths(bsdb_db *db, uint64_t count, const uint32_t *d_klen, const uint32_t *d_vlen,
                             uint8_t *d_status, uint32_t *d_llen, uint64_t *d_loff, void *stream);
int bsdb_dev_db_dump_text(bsdb_db *db, uint64_t count, const uint64_t *d_ksrc, const uint32_t *d_klen,
                          const uint64_t *d_vsrc, const uint32_t *d_vlen, const uint32_t *d_llen, const uint64_t *d_loff,
                          int separator, uint8_t *d_text, uint64_t text_bytes, uint8_t *d_status, uint64_t first,
                          uint64_t *d_report /* BSDB_SCAN_WORDS */, void *stream);
int bsdb_db_set_text_chunk(bsdb_db *db, uint64_t bytes);
int bsdb_db_scan(bsdb_db *db, uint64_t first, uint64_t count, uint64_t key_cap, uint64_t value_cap, uint8_t *h_keys,
                 uint64_t *h_koff, uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status,
                 uint64_t *report /* BSDB_SCAN_WORDS */);
int bsdb_db_dump_text(bsdb_db *db, const char *path, int separator, uint64_t first, uint64_t count, int append,
                      uint64_t *report /* BSDB_SCAN_WORDS */);

/* ---- two resident databases compared: same, changed, absent ----------------
 * What changed between database A and database B, both resident on one
 * context: every slot of A gets one status byte that says what B holds for
 * that slot's key.  A's records are listed by slot (bsdb_dev_db_records), their
 * keys packed (bsdb_dev_edge_offsets + bsdb_dev_db_gather) and located in B
 * (bsdb_dev_db_locate_var); the values are then compared in place, image
 * against image: nothing is gathered, and no record passes through host memory
 * unless it is written to a delta file.  (The reference has no diff.)  Exact
 * mode only.
 *
 * A slot's status:
 *   0 BSDB_DIFF_SAME          B holds the key with the same value length and bytes
 *   1 BSDB_GET_REJECTED       B's MPHF rejects the key: absent from B
 *   2 BSDB_GET_KEY_MISMATCH   B's slot holds another key: absent from B
 *   3 BSDB_GET_BAD_ADDR       B's slot names no whole record: B is damaged
 *   4 BSDB_CHECK_VALUE_LEN    present in both, the value lengths differ
 *   5 BSDB_CHECK_VALUE_BYTES  present in both, the same length, some byte differs
 *   6 BSDB_DIFF_BAD_SLOT      A's own slot names no record (BSDB_SCAN_BAD_ADDR
 *                             from bsdb_dev_db_records); it is not looked up
 * The report is uint64_t[BSDB_DIFF_WORDS], ACCUMULATED by the dev_ call into
 * words the caller zeroed, with [8] = UINT64_MAX:
 *   [0] slots   [1] same   [2] rejected   [3] key_mismatch   [4] bad_addr
 *   [5] value_len   [6] value_bytes   [7] bad_slot     [0] == [1] + ... + [7]
 *   [8] first_diff: the lowest slot of A that is not SAME, UINT64_MAX when none
 *   [9] compared_bytes: the sum of the value lengths actually compared
 *
 * bsdb_dev_db_diff: d_vsrc_a / d_vlen_a / d_status_a are bsdb_dev_db_records'
 *   on A for slots [slot_base, slot_base + count), d_src_b / d_vlen_b what
 *   bsdb_dev_db_locate_var on B returned for those records' keys; d_status
 *   comes in as locate's and goes out as the diff's (a byte that is none of
 *   locate's counts as BAD_ADDR).  All descriptor arrays are data: no byte
 *   outside image A is read through A's positions and none outside image B
 *   through B's (a position past its image reads as 0), and a length over
 *   65 535 is VALUE_LEN, never compared.  The workspace is the context's.
 *   Asynchronous.
 * bsdb_dev_db_select: the records whose status bit is set in `mask` (bit s
 *   selects status s; bit 6 or any higher bit is BSDB_EINVAL: a BAD_SLOT has
 *   no record to write), in slot order: d_sel[j] (u64) the index in
 *   [0, count) of the j-th selected record, d_*_out[j] its four descriptors,
 *   *d_nsel (one u64) how many there are; every output array holds `count`
 *   entries.  The outputs feed bsdb_dev_db_dump_lengths and
 *   bsdb_dev_db_dump_text unchanged, with a zeroed status array.  No cursor
 *   atomics: the output is deterministic.  Asynchronous.
 * bsdb_db_diff: the whole comparison in both directions, A -> B over all of
 *   A's slots, then B -> A over all of B's, each in chunks of bsdb_db_set_batch
 *   slots of the side that is listed; never more than one chunk is held.
 *   removed_path receives the lines key<sep>value of A's records whose A -> B
 *   status is 1 or 2, in A's slot order; upsert_path those of B's records whose
 *   B -> A status is 1, 2, 4 or 5 (added or changed), in B's slot order; a
 *   chunk's text is written in pieces under the cap of bsdb_db_set_text_chunk
 *   of the side that is listed.  `bsdb_text_build` and `bsdb_db_check_text`
 *   read such lines.  Either path may be NULL: the two diff reports are still
 *   complete.  scan_upsert / scan_removed are the dump's reports
 *   (BSDB_SCAN_WORDS) of the two files: [0] the lines written, [3] not_text
 *   whether the text carries every record, [7] the first such line of the
 *   file; empty for a NULL path.  Returns BSDB_OK whatever the statuses.
 *   Two verified databases give report_ab[1] == report_ba[1], [5] == [5] and
 *   [6] == [6].
 * All: BSDB_EINVAL before any device call for null or misaligned arguments, an
 *   approximate database on either side, two databases that are not on the
 *   same context, one whose MPHF was freed, or a bad separator; BSDB_EFILE for
 *   a file that cannot be written; count == 0 and n == 0 are BSDB_OK with zero
 *   counts.
 * Out of scope: approximate databases, databases on different devices, two
 * databases that do not fit the device together (bsdb_db_open answers
 * BSDB_ENOMEM), and compressed kv.db.  Applying a delta is the next block's
 * (bsdb_db_merge).
 * ------------------------------------------------------------------------- */
#define BSDB_DIFF_WORDS 10
#define BSDB_DIFF_SAME 0
#define BSDB_DIFF_BAD_SLOT 6
int bsdb_dev_db_diff(bsdb_db *a, bsdb_db *b, uint64_t count, const uint64_t *d_vsrc_a, const uint32_t *d_vlen_a,
                     const uint8_t *d_status_a, const uint64_t *d_src_b, const uint32_t *d_vlen_b, uint8_t *d_status,
                     uint64_t slot_base, uint64_t *d_report /* BSDB_DIFF_WORDS */, void *stream);
int bsdb_dev_db_select(bsdb_db *db, uint64_t count, const uint8_t *d_status, uint32_t mask, const uint64_t *d_ksrc,
                       const uint32_t *d_klen, const uint64_t *d_vsrc, const uint32_t *d_vlen, uint64_t *d_sel,
                       uint64_t *d_ksrc_out, uint32_t *d_klen_out, uint64_t *d_vsrc_out, uint32_t *d_vlen_out,
                       uint64_t *d_nsel, void *stream);
int bsdb_db_diff(bsdb_db *a, bsdb_db *b, int separator, const char *upsert_path, const char *removed_path,
                 uint64_t *report_ab /* BSDB_DIFF_WORDS */, uint64_t *report_ba /* BSDB_DIFF_WORDS */,
                 uint64_t *scan_upsert /* BSDB_SCAN_WORDS */, uint64_t *scan_removed /* BSDB_SCAN_WORDS */);

/* ---- resident databases merged into a new directory: delta over base -------
 * merge(base, delta, removed) -> new kv.db files + index files.  All three are
 * exact databases resident on one context; delta and removed may be NULL.  The
 * output holds every record of delta, and every record of base whose key
 * neither delta nor removed holds.  Of removed only the keys matter; a key in
 * both delta and removed is in the output with delta's value.  With delta and
 * removed NULL the call is a rebuild: the same records into another partition
 * count, layout, signature width or approximate mode.  No record passes
 * through text: a record whose key or value holds the separator, LF or CR
 * (BSDB_SCAN_NOT_TEXT) is carried like any other.  (The reference has no
 * merge.)
 *
 * Record order: base's kept records in base's slot order, then delta's in
 * delta's slot order.  The records one pack writes are cut into `partitions`
 * runs by bsdb_text_build's rule (run p = records [p k / P, (p + 1) k / P)) and
 * appended to kv.db.<p>, in the layout bsdb_text_build_layout writes.
 *
 * A slot of base gets one status byte:
 *   0 BSDB_MERGE_KEPT       it goes on
 *   1 BSDB_MERGE_REPLACED   delta holds the key (locate: BSDB_GET_FOUND)
 *   2 BSDB_MERGE_REMOVED    removed holds it and delta does not
 *   3 BSDB_MERGE_BAD_SLOT   base's own slot names no record (BSDB_SCAN_BAD_ADDR);
 *                           it has no key and is not looked up
 *   4 BSDB_MERGE_BAD_ADDR   locate in delta or in removed returned
 *                           BSDB_GET_BAD_ADDR, or a status byte that is no code;
 *                           it wins over what the other database answers
 * BSDB_GET_REJECTED and BSDB_GET_KEY_MISMATCH both mean absent.
 * The report is uint64_t[BSDB_MERGE_WORDS], ACCUMULATED by the dev_ calls into
 * words the caller zeroed:
 *   [0] base_slots  [1] kept  [2] replaced  [3] removed  [4] bad_slot
 *   [5] bad_addr    [6] delta_slots  [7] delta_written  [8] delta_bad_slot
 *   [9] out_records [10] out_key_bytes  [11] out_value_bytes
 *   [0] == [1] + ... + [5] and, for bsdb_db_merge, [9] == [1] + [7], for any
 *   input.
 *
 * bsdb_dev_db_merge_status: d_status_base is bsdb_dev_db_records' status of
 *   base's slots, d_status_delta / d_status_removed what
 *   bsdb_dev_db_locate_var returned for those records' keys in delta / removed
 *   (either may be NULL: that database is not there); d_status_out gets the
 *   merge's status, words [0] .. [5] of d_report the counts.  Its output feeds
 *   bsdb_dev_db_select with mask 1 << BSDB_MERGE_KEPT.  Asynchronous.
 * bsdb_dev_db_pack: `count` records of db's resident image, named by the
 *   descriptors bsdb_dev_db_records or bsdb_dev_db_select gave, into the image
 *   of a kv.db chunk: the argument list and the outputs of bsdb_dev_text_pack
 *   (format 0) / bsdb_dev_text_pack_blocked (format 1, block_size), byte for
 *   byte what those write for the same records, with the same refusals
 *   (BSDB_EINVAL for misaligned descriptor or output arrays, a bad block size,
 *   h_part_size no multiple of 4096 for the blocked layout, and -- after the
 *   sizes are known, before anything is written -- an image or key blob over
 *   its cap; bsdb_text_image_max does not apply: 16 + the records' bytes hold a
 *   compact image, 16 + twice that + partitions x block_size a blocked one).
 *   Positions are u64 at any alignment.  Every position and length is data: a
 *   length is cut to 255 (key) / 32 510 (value) wherever it is used, a position
 *   at or past the image's end reads as zeros, and nothing is written outside
 *   the caller's buffers.  Waits once, for the sizes.
 * bsdb_db_merge: the whole merge.  base in chunks of bsdb_db_set_batch slots:
 *   records, keys gathered, located in delta and in removed, status, select,
 *   then the selection in packs whose image stays under base's
 *   bsdb_db_set_text_chunk cap (a single record above it goes alone), each
 *   image to the host, its runs appended to kv.db.<p>, its records added to a
 *   streaming builder on the device; then delta in chunks of its own setting,
 *   every record written; then bsdb_builder_finish writes index_path (and
 *   index_a_path when `approximate`, which must then be given) with
 *   `width` = hash.checksum.bits.  A merge must not lose records silently: if
 *   bad_slot, bad_addr or delta_bad_slot is non-zero after a chunk, the call
 *   stops there with BSDB_EVERIFY, the report filled up to that chunk and no
 *   index file written (the kv.db files are incomplete).  Values over 32 510
 *   bytes, which no writer of this project produces, are cut to that length.
 * All: BSDB_EINVAL before any device call for null or misaligned arguments, an
 *   approximate input, inputs on different contexts, one whose MPHF was freed,
 *   bad partitions, format or block size, `approximate` without index_a_path;
 *   BSDB_EFILE for a file that cannot be written.
 * Out of scope: compressed kv.db, approximate inputs, inputs that do not fit
 * one device together, more than one delta per call.
 * ------------------------------------------------------------------------- */
#define BSDB_MERGE_WORDS 12
#define BSDB_MERGE_KEPT 0
#define BSDB_MERGE_REPLACED 1
#define BSDB_MERGE_REMOVED 2
#define BSDB_MERGE_BAD_SLOT 3
#define BSDB_MERGE_BAD_ADDR 4
int bsdb_dev_db_merge_status(bsdb_ctx *ctx, uint64_t count, const uint8_t *d_status_base, const uint8_t *d_status_delta,
                             const uint8_t *d_status_removed, uint8_t *d_status_out,
                             uint64_t *d_report /* BSDB_MERGE_WORDS */, void *stream);
int bsdb_dev_db_pack(bsdb_ctx *ctx, bsdb_db *db, const uint64_t *d_ksrc, const uint32_t *d_klen, const uint64_t *d_vsrc,
                     const uint32_t *d_vlen, uint64_t count, int partitions, int format, uint32_t block_size,
                     const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap, uint64_t *h_run_bytes,
                     uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off, uint64_t *h_blob_bytes,
                     uint64_t *d_value8, uint8_t *d_value_len, void *stream);
int bsdb_db_merge(bsdb_db *base, bsdb_db *delta, bsdb_db *removed, const char *kv_base, int partitions, int format,
                  uint32_t block_size, uint32_t width, int approximate, const char *index_path, const char *index_a_path,
                  uint64_t *report /* BSDB_MERGE_WORDS */, bsdb_mph **out);

#ifdef __cplusplus
}
#endif
#endif /* BSDB_MI355X_H */
