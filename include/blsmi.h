/*
 * blsmi.h -- C ABI of libblsmi.so: MI355X-native batch BLS12-381 engine behind the
 * g1pubs / g2pubs Verify / VerifyAggregate surface of phoreproject/bls.
 *
 * This is the drop-in boundary: the entry points are what a cgo shim in the reference's Go
 * packages would bind (see INTEGRATION.md for the Go side).  Plain pointers and sizes only.
 *
 * Conventions
 *   - Host entry points (no suffix) take HOST pointers, are blocking and re-entrant; the library
 *     owns device memory and streams.  `_dev` entry points take DEVICE pointers (inputs already
 *     resident in HBM) plus a hipStream_t passed as void* (NULL = the library's stream); the work is
 *     enqueued on that stream and the call returns after synchronising it (results are ready).
 *   - Field elements on the wire are 48-byte big-endian normal form, exactly
 *     G1Affine.SerializeBytes / G2Affine.SerializeBytes of the reference
 *     (g1.go:157-167: x||y, 96 B; g2.go:172-186: x.c0||x.c1||y.c0||y.c1, 192 B).
 *   - Fq12 results are 72 little-endian uint64 per element: the reference's in-memory FQ12
 *     (Montgomery form R = 2^384, coefficient order c0.c0.c0, c0.c0.c1, ... c1.c2.c1 --
 *     pairing_test.go:9-20), bit for bit.
 *   - Scalars are 32-byte big-endian (FRRepr.Bytes, frrepr.go:188-195).
 *   - Return value: 0 on success, negative BLSMI_E_* on error.  Where the reference panics
 *     (a point at infinity entering MillerLoop, pairing.go:17-26/54) the library never aborts:
 *     the tuple gets a defined result (verify -> 0 / false, pairing -> 1) -- see each function.
 */
#ifndef BLSMI_H
#define BLSMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLSMI_OK 0
#define BLSMI_E_NODEVICE (-1)   /* no usable HIP device */
#define BLSMI_E_HIP (-2)        /* a HIP runtime call failed */
#define BLSMI_E_ARG (-3)        /* bad argument (null pointer with n > 0, ...) */
#define BLSMI_E_NOMEM (-4)
#define BLSMI_E_RCCL (-5)       /* librccl could not be loaded, or a collective failed (multi-GPU only) */
#define BLSMI_E_RNG (-6)        /* the OS random source (getrandom, /dev/urandom) failed: no scalars were drawn (blsmi 0.8, *_verify_batch_rlc) */

/* Bind the calling process to ONE device (HIP ordinal >= 0) and create the library's streams and tables.
 * Idempotent; every other host entry point calls it lazily with device 0. */
int blsmi_init(int device);
/* Drive the first `ndev` devices of this node from this one process (ndev <= 0: every visible device).  Large
 * verify / pairing batches are then split by contiguous block over the devices -- one host thread, stream context
 * and memory pool per shard -- so a single call to blsmi_g{1,2}pubs_verify_batch / _verify_aggregate /
 * blsmi_pairing_batch uses all of them; the only exchanges are the pass/fail bitmap (one RCCL all-reduce over
 * xGMI) and, for an n-way VerifyAggregate, the per-device Fq12 partial products (one RCCL all-gather of 720 bytes
 * per device).  Smaller calls go to the least busy device.  Must be the first call (or repeat the same ndev).
 * Environment: BLSMI_SHARDS (logical shards, default ndev; more shards than devices share devices),
 * BLSMI_SHARD_MIN (smallest batch that is split, default 8192), BLSMI_FORCE_RCCL=1 (build the communicator even
 * for one device).  librccl is loaded with dlopen only when ndev > 1 (or forced) -- BLSMI_RCCL_PATH names the file to load when the
 * process' loader path has none (a Go binary; under torch one is already mapped) --: BLSMI_E_RCCL if that fails. */
int blsmi_init_devices(int ndev);
/* TEST HOOK, not a deployment mode.  With BLSMI_DEVICE_ALIAS=0,0[,0,0] in the environment blsmi_init_devices builds that many LOGICAL
 * devices -- each with its own context pool, streams, generator tables and exchange buffer, as on an N-GPU node -- on the physical GPUs
 * the list names (ndev <= 0: as many as the list has), and, because RCCL refuses two ranks on one GPU, runs the two collectives through
 * a host-staged stand-in with the same buffers and results (blsmi_version() then says ALIASED-DEVICES).  It exists so that a one-GPU
 * box executes the multi-device code: shard -> device routing, per-device pools, owner routing of the *_dev entry points.
 * blsmi_debug_alias_own tells the library which logical device "owns" a device-pointer range (on real hardware the HIP runtime
 * answers that; aliased devices share one ordinal); bytes == 0 forgets the range.  BLSMI_E_ARG outside the hook. */
int blsmi_debug_alias_own(const void *d_ptr, size_t bytes, int device_index);
int blsmi_device_count(void);   /* devices in use (0 before initialisation) */
/* Diagnostic: context leases (entry-point calls + shards of split calls) that device `device_index` (0 .. blsmi_device_count() - 1) has
 * served since initialisation; -1 for no such device.  Lets an operator (and the tests) see that work reaches every device. */
long long blsmi_debug_device_leases(int device_index);
int blsmi_shard_count(void);
void blsmi_shutdown(void);
/* "blsmi <ABI version> gfx950 CUs=.. devices=.. shards=..".  ABI history: 0.2 gave blsmi_g{1,2}pubs_aggregate_partial its trailing
 * `int *bad` argument (a caller built against the 5-argument prototype of 0.1 must be rebuilt); 0.3 adds the *_dev forms of
 * mul / sum / msm / verify_aggregate and changes no existing prototype; 0.4 adds the prepared-key entry points.  Check the prefix
 * before binding by hand.  0.5 adds blsmi_trim / blsmi_held_bytes, the *_ex forms of mul / msm (per-call BLSMI_MUL_ANY_POINT),
 * blsmi_prefer_cpu, blsmi_debug_device_leases and the BLSMI_DEVICE_ALIAS test hook; no existing prototype changes.  0.6 adds the *_jac forms
 * (the reference's in-memory Jacobian / Montgomery points at the boundary); no existing prototype changes.  0.7 adds blsmi_set_row_threshold (the lane-row layout for
 * 2 048 .. 8 192 tuples), the "row_side" / "hash_row_min" / "hash_row_max" / "hash_quad_min" / "hash_quad_max" / "hash_oct_min" / "hash_oct_max" / "hash_g1_quad_min" / "hash_g1_quad_max" options and BLSMI_OP_LANE_ROW / BLSMI_OP_ROW_*_STEP / BLSMI_OP_ROW_G2_* / BLSMI_OP_ROW_CLEAR_H2 for blsmi_debug_op; no existing prototype changes.  0.8 adds the randomised batch verification (blsmi_g?pubs_*verify*_batch_rlc[_jac]),
 * the "rlc_min" option, BLSMI_E_RNG and BLSMI_OP_G1_MUL_U64; no existing prototype changes.  0.9 adds the segmented sums (blsmi_g?_sum_segmented[_jac|_dev]),
 * the batches of VerifyAggregateCommon over key committees (blsmi_g?pubs_verify_aggregate_common*_batch[_jac|_dev]) and the "segsum_chunk" option;
 * no existing prototype changes.  0.10 adds the pairing products (blsmi_pairing_product_batch[_jac|_dev|_jac_dev]: many MillerLoop(items) + FinalExponentiation
 * checks in one call); no existing prototype changes, no new option.  0.11 adds the grouped randomised batch verification
 * (blsmi_g?pubs_*verify*_batch_rlc_grouped[_jac]: the tuples of one message share one pairing) and the weighted segmented sums
 * (blsmi_g?_sum_segmented_u64); no existing prototype changes, no new option.  0.12 adds the randomised batch verification that
 * finds the bad tuples by blocks (blsmi_g?pubs_*verify*_batch_rlc_locate[_jac]); no existing prototype changes, no new option.  0.13 adds the grouped
 * randomised batch verification that finds the bad tuples by cells (blsmi_g?pubs_*verify*_batch_rlc_grouped_locate[_jac]); no existing prototype
 * changes, no new option.  0.14 adds the batch point validation (blsmi_g?_check_batch[_jac|_dev]: on-curve and subgroup status of points in either
 * form, no inversion, no square root) and the BLSMI_POINT_* status names; no existing prototype changes, no new option.  0.15 adds the conversions between the compressed wire format and the in-memory points
 * (blsmi_g?_decompress_batch_jac[_dev], blsmi_g?_compress_batch_jac[_dev]); no existing prototype changes, no new option.  0.16 adds the randomised
 * verification of many committee aggregates in one call (blsmi_g?pubs_verify_aggregate_common*_batch_rlc[_jac|_dev]) and
 * blsmi_debug_g2_sum_segmented_u64_pair; no existing prototype changes, no new option.  0.17 adds the randomised pairing-product batches
 * (blsmi_pairing_product_batch_rlc[_jac|_dev|_jac_dev]: one equation for a batch of pairing products, the pairs of one G2 table entry sharing
 * one Miller loop) and blsmi_debug_pairing_product_batch_rlc_dev_nosplit; no existing prototype changes, no new option.  0.18 adds the randomised pairing-product
 * batches that find the bad items by blocks (blsmi_pairing_product_batch_rlc_locate[_jac|_dev|_jac_dev]); no existing prototype changes, no
 * new option.  0.19 adds arithmetic mod r -- the weighted segmented fold of scalars (blsmi_fr_wsum_segmented_u64[_dev]) -- and the Groth16
 * batches that fold their public inputs with it (blsmi_groth16_verify_batch[_jac|_dev|_jac_dev]); no existing prototype changes, no new
 * option.  0.20 adds the lift out = A + k * B in G1 (blsmi_g1_mul_add_batch[_dev]) and the KZG batches that fold their values mod r
 * (blsmi_kzg_verify_batch[_jac|_dev|_jac_dev]); no existing prototype changes, no new option.  0.21 adds the scalar field proper --
 * products and inverses mod r (blsmi_fr_mul_batch[_dev], blsmi_fr_inv_batch[_dev]) --, the evaluation of polynomials in evaluation form
 * (blsmi_fr_eval_batch[_dev]) and the KZG blob batches that evaluate their blobs with it (blsmi_kzg_verify_blob_batch[_jac|_dev|_jac_dev]);
 * no existing prototype changes, no new option.  0.22 adds the interpolation of a polynomial from its values over a coset
 * (blsmi_fr_coset_interp_batch[_dev]) and the KZG cell batches that interpolate their cells with it
 * (blsmi_kzg_verify_cell_batch[_jac|_dev|_jac_dev]); no existing prototype changes, no new option.  0.23 adds the Fiat-Shamir challenge of
 * a blob proof (blsmi_kzg_blob_challenge_batch[_dev]) and the KZG blob batches from wire bytes that derive it, decompress their points and
 * apply EIP-4844's verdict rules (blsmi_kzg_verify_blob_batch_wire[_dev]), with blsmi_debug_kzg_blob_challenge_form_dev and
 * blsmi_debug_kzg_verify_blob_batch_wire_dev_serial; no existing prototype changes, no new option.  The string below
 * still begins "blsmi 0.10": a caller that binds by hand tells 0.11, 0.12, 0.13, 0.14, 0.15, 0.16, 0.17, 0.18, 0.19, 0.20, 0.21, 0.22 and 0.23
 * by the presence of those symbols. */
const char *blsmi_version(void);

/* Page-locked ("pinned") host memory for the buffers handed to the host entry points below.  Optional: every entry point takes
 * ordinary (pageable) memory, which the HIP runtime stages at ~10 GB/s; from blsmi_host_alloc memory the copies are single DMAs at
 * PCIe rate (65 536 pairings from host buffers: 26 -> 22 ms).  A cgo caller serialises its points straight into such a buffer
 * (INTEGRATION.md 2e).  The memory is visible to every device the library drives. */
/* Device memory held for future calls.  Every call context (BLSMI_STREAMS per device) keeps the temporaries of its last call for reuse
 * -- steady state makes no allocator call at all -- up to a retention cap of BLSMI_ARENA_KEEP_MB (default 4096) per context: what an
 * outsized call needed beyond the cap is returned to the driver when that call ends.  blsmi_trim gives back what IDLE contexts hold
 * beyond keep_bytes_per_context (0: everything) plus the runtime's pool cache, e.g. after a burst of 2^20-point calls or before another
 * library in the process needs the HBM; *freed_bytes (may be NULL) reports how much.  blsmi_held_bytes: the current total. */
int blsmi_trim(size_t keep_bytes_per_context, size_t *freed_bytes);
size_t blsmi_held_bytes(void);
int blsmi_host_alloc(size_t bytes, void **out);
int blsmi_host_free(void *p);

/* ---- pairing (replaces bls.Pairing, pairing.go:132-136; BASELINE config 2) -------------------
 * out[i] = FinalExponentiation(MillerLoop(P_i, Q_i)) for n independent (P_i in G1, Q_i in G2)
 * affine pairs.  Inputs must be finite curve points (the reference panics on infinity). */
int blsmi_pairing_batch(const uint8_t *g1_aff /* n*96 */, const uint8_t *g2_aff /* n*192 */,
                        uint64_t *out_fq12 /* n*72 */, size_t n);
int blsmi_pairing_batch_dev(const void *d_g1_aff, const void *d_g2_aff, void *d_out_fq12, size_t n, void *stream);
/* Per-kernel HIP-event timing of the last blsmi_pairing_batch[_dev] call (used by bench.py for the
 * roofline object): Miller-loop kernel and final-exponentiation kernel durations in milliseconds. */
int blsmi_set_profiling(int on);
/* Latency path: pairing / verify batches of at most `max_tuples` tuples run ONE TUPLE PER WAVE (the pairing spread over
 * 64 lanes, field elements staged in LDS) instead of one per lane pair: ~10x lower latency for the one-tuple-per-call
 * Go API (g2pubs/bls.go:159-162), same results.  Default 8192 (environment BLSMI_LAT_MAX) -- the two paths cross at ~10 000 tuples --; 0 switches it off. */
int blsmi_set_latency_threshold(size_t max_tuples);
/* Mid-size batches: pairing / verify batches above the latency threshold and of at most `max_tuples` tuples run in the LANE-QUAD layout
 * -- four lanes per tuple, 16 384 tuples = one wave on every SIMD of the chip -- instead of the lane-pair layout, which needs 65 536
 * tuples to fill it (16 384 pairings: 11.5 ms there).  Default 16 384 (environment BLSMI_QUAD_MAX); 0 switches the layout off.
 * Same results bit for bit on all paths. */
int blsmi_set_quad_threshold(size_t max_tuples);
/* A few thousand tuples (blsmi 0.7): a LONE pairing / verify call of min_tuples .. max_tuples tuples runs in the LANE-ROW layout -- sixteen lanes (one DPP
 * row) per tuple, 4 096 tuples = one wave on every SIMD of the chip -- instead of one tuple per wave (below) or per lane quad (above).  Default
 * 2 048 .. 8 192 (environment BLSMI_ROW_MIN / BLSMI_ROW_MAX); max_tuples = 0 switches the layout off.  Calls that find other calls in flight on
 * their device keep the quad kernels (see "crowd_quad" below).  Same results bit for bit on all four paths. */
int blsmi_set_row_threshold(size_t min_tuples, size_t max_tuples);
/* When should a lone call stay on the upstream CPU path?  A call with few elements costs the dependent depth of ONE wave walking the
 * whole computation -- about 0.7 ms for a Miller loop, 1.4 ms for a pairing, a signature or a G2 preparation, 2.0 ms for a Verify --
 * whatever n is, up to a few thousand elements.  Where one CPU core needs less than that for the whole call (BLSSign 0.45 ms,
 * G2AffineToPrepared 0.19 ms, a Jacobian addition 6.5 us: bench.py `reference_shapes`), the shim should not cross the boundary.
 * blsmi_prefer_cpu(shape, n) returns 1 in exactly those cases (n * cpu time per operation < device latency of a lone call), else 0:
 * Sign n <= 3, G2 prepare n <= 7, MillerLoop n = 1, point sums n <= 38; never for Pairing / FinalExponentiation / Verify. */
enum { BLSMI_SHAPE_PAIRING = 0, BLSMI_SHAPE_MILLER_LOOP = 1, BLSMI_SHAPE_FINAL_EXP = 2, BLSMI_SHAPE_G2_PREPARE = 3, BLSMI_SHAPE_VERIFY = 4,
       BLSMI_SHAPE_SIGN = 5, BLSMI_SHAPE_VERIFY_DOMAIN = 6, BLSMI_SHAPE_POINT_ADD = 7 };
int blsmi_prefer_cpu(int shape, size_t n);
/* Environment.  Every BLSMI_* variable is read ONCE, when the library initialises (the first entry point, blsmi_init or blsmi_init_devices),
 * never from an entry point afterwards: changing the environment of a running process changes nothing (and getenv racing setenv is undefined
 * behaviour in a threaded host).  An option set through the API (blsmi_set_option, blsmi_set_*) before or between initialisations keeps its value; every
 * other takes its variable's value, or its default where the variable is unset.  Each option, its variable and the rule the variable is read by are one
 * row of the table `options` in bls_amd/csrc/route.h.  Deployment: BLSMI_STREAMS (call contexts per device, 4), BLSMI_SHARDS, BLSMI_SHARD_MIN, BLSMI_FORCE_RCCL,
 * BLSMI_RCCL_PATH (the librccl to dlopen when several devices are driven -- a Go binary has no torch that maps one), BLSMI_ARENA_KEEP_MB,
 * BLSMI_LAT_MAX / BLSMI_QUAD_MAX / BLSMI_QUAD_MIN (layout hand-overs; also blsmi_set_latency_threshold / _quad_threshold), BLSMI_MUL_GENERIC,
 * BLSMI_COMBINE_MAX / _WAIT_US / _INFLIGHT / _DEBUG (merging of concurrent one-tuple Verify calls).  A/B switches between code paths with
 * identical results (held to the oracle by tests/test_gpu_startup_switches.py): BLSMI_LAYOUT, BLSMI_GEN_LINES, BLSMI_HASH_G1_SPLIT, BLSMI_HASH_G2_PAIR, BLSMI_HASH_G2_PAIR_REDO_EVERY, BLSMI_COFAC2_PAIR,
 * BLSMI_SWU_WAVE_MAX, BLSMI_SIG_SIDE_MAX, BLSMI_SIDE_MAX, BLSMI_FIXED_WAVE_MAX, BLSMI_MSM_BUCKET_MIN, and the ones that can ALSO be
 * switched while running through blsmi_set_option(name, value) (as the thresholds above: every call reads every option ONCE, when it starts,
 * so a change applies to the calls that start after it and never to part of a call in flight):
 *   "agg_cofactor_pow" (BLSMI_AGG_COFACTOR_POW, default 1), "msm_sort" (BLSMI_MSM_SORT, default 1), "dup_force_sort" (BLSMI_DUP_FORCE_SORT, 0),
 *   "rlc_min" (BLSMI_RLC_MIN, default 32768): the randomised batch verification (*_verify_batch_rlc) of fewer tuples runs the per-tuple path,
 *   "segsum_chunk" (BLSMI_SEGSUM_CHUNK, default 0 = automatic: 8, doubled up to 64 while more than 2^16 chunks would remain): positions per lane of
 *   the segmented sums (blsmi_g?_sum_segmented, the *_verify_aggregate_common*_batch entry points) and values per lane row of the pairing products' segmented
 *   Fq12 product (blsmi_pairing_product_batch*),
 *   "lat_rolled" (BLSMI_LAT_ROLLED, default 1; 0: small Pairing calls run the straight-line copy of their level program instead of the one
 *   whose squaring runs are loops), "row_side" (BLSMI_ROW_SIDE, default 1: a Verify in the row layout runs its signature side beside the hash -- g1pubs, and g2pubs with "row_side_g2pubs"),
 *   "hash_row_min" / "hash_row_max" (defaults 2048 / 4096; no environment name): HashG2 of that many messages clears its cofactor sixteen lanes per message
 *   (k_hash_g2_front + k_clear_h2_row, 2.9 -> 2.2 ms for 3 072 messages) instead of a lane pair per message; "hash_quad_min" / "hash_quad_max" (4097 / 16384):
 *   four lanes per message (k_clear_h2_quad, 3.0 -> 2.4 ms for 16 384 messages: 16 384 g1pubs verifies 10.1 -> 9.3 ms); max 0: never.
 *   "hash_oct_min" / "hash_oct_max" (2048 / 7168): EIGHT lanes per message (k_clear_h2_oct: the homogeneous formulas' levels are four and six products wide; takes precedence
 *   over the two above where its range covers the count: 4 096 g1pubs verifies 4.45 -> 4.05 ms, 6 144: 6.54 -> 5.94).
 *   "swu_row_max" (4096): the SWU maps of HashG1 / HashG2 of BLSMI_SWU_WAVE_MAX < n <= swu_row_max messages run a row of sixteen lanes per map (k_swu_g?_rows:
 *   k_swu_g1 0.54 -> 0.24 ms up to 2 048 messages) unless the signature side's kernel runs beside the hash; 0: never.
 *   "row_side_g2pubs" (1): g2pubs too (its side kernel over the generator's prepared lines, the hash's maps a lane each beside it: 4 096 g2pubs verifies
 *   3.23 against 3.55 ms in the two-pair loop, 8 192: 5.37 against 5.71; 0: the two-pair loop).
 *   "hash_g1_quad_min" / "hash_g1_quad_max" (1280 / 32768): HashG1 of that many messages runs its tail -- sum, 11-isogeny, cofactor -- four lanes per message
 *   (k_hash_g1_finish_quad: 0.96 -> 0.48 ms; 4 096 g2pubs verifies 4.35 -> 3.78 ms, 16 384: 8.10 -> 7.57 ms).
 * Layout by what the DEVICE carries (blsmi 0.6): the hand-overs above are a lone caller's.  Calls that arrive together share the chip, and
 * under load the quad kernels serve 2.7x the tuples per second of the one-tuple-per-wave path, so a pairing / verify call of at least
 * "crowd_floor" tuples (BLSMI_CROWD_FLOOR, default 1536) takes them when its tuples plus those of the other calls in flight on its device pass
 * BLSMI_QUAD_MIN; "crowd_quad" (BLSMI_CROWD_QUAD, default 1) 0: by the call's own size only.  Same results either way (bit-exact layouts).
 * Concurrent Verify calls of BLSMI_COMBINE_MAX <= n < "combine_mid_max" tuples (BLSMI_COMBINE_MID_MAX, default 8192; 0: never) are merged into one
 * launch among themselves when no call context is free (more callers than BLSMI_STREAMS), like the one-tuple calls below BLSMI_COMBINE_MAX are among
 * theirs.
 * Eight callers x 4 096 g2pubs tuples: 0.73 -> 1.84 M verifies/s with both; four callers x 4 096 pairings: 1.04 -> 2.50 M/s.
 * Concurrency needs hardware queues: the HIP runtime hands its GPU_MAX_HW_QUEUES queues (default 4) to streams in creation order and kernels of one
 * queue run one after the other, so the library creates its call contexts' streams back to back when it initialises (BLSMI_STREAMS = 4 = one queue
 * each).  Supported ceiling (round 6, profiles/r06_queue_matrix.log): BLSMI_STREAMS <= 4 -- the default -- at ANY GPU_MAX_HW_QUEUES (4, 6, 8 measured: 0.73 - 1.18 M verifies/s for 4 - 16 callers).
 * More call contexts than four on more than four hardware queues collapse (0.14 - 0.30 M verifies/s) or abort inside the runtime: HSA_STATUS_ERROR_OUT_OF_RESOURCES -- a hardware queue's scratch is sized
 * for a chip full of waves of the largest private segment it has dispatched (k_cofac2_pair: 7 680 bytes a lane, ~4 GB a queue), and eight such queues are more than the runtime grants
 * (profiles/r06_queue_abort_q8_c8.log).  Callers beyond four merge or wait.
 * Test hooks: BLSMI_DEVICE_ALIAS (above); "assume_load" (tuples pretended to be in flight from other calls).  Unknown option name: BLSMI_E_ARG.  (blsmi 0.6) */
int blsmi_set_option(const char *name, long long value);
int blsmi_last_kernel_ms(float *miller_ms, float *final_exp_ms);
/* General form: with profiling on, every entry point records HIP events on its launch stream between its major kernels.  This
 * returns the calling thread's log since it last asked, as "kernel=ms;kernel=ms;..." in launch order (a name repeats when a
 * kernel is launched several times; "k_lat:<program>" = a level program of the latency path), and clears it.  Return value:
 * the length needed.  Only unsplit calls are logged (the shard threads of a split call keep their own logs). */
int blsmi_last_profile(char *out, size_t cap);
/* Miller loop only (pairing.go:16-75 with one pair per tuple), same output format */
int blsmi_miller_loop_batch(const uint8_t *g1_aff, const uint8_t *g2_aff, uint64_t *out_fq12, size_t n);
/* Final exponentiation only (pairing.go:79-129) on n Fq12 values in the output format.  Zero, the one value without an inverse, has no
 * result in the reference (nil, pairing.go:83); here it gives the zero Fq12, on every layout (wave, row, single lane, and the pair / quad
 * kernels of BLSMI_OP_FQ12_FINAL_EXP), since zero times the inversion's output is zero in the easy part. */
int blsmi_final_exponentiation_batch(const uint64_t *in_fq12, uint64_t *out_fq12, size_t n);

/* ---- scalar multiplication and point sums (g1.go:80-90, g2.go:92-102, AggregatePublicKeys /
 * AggregateSignatures g2pubs/bls.go:165-192; BASELINE config 3) --------------------------------
 * out[i] = k_i * P_i in affine form; out_inf[i] = 1 when the result is the point at infinity
 * (its 96/192 bytes are then zero).  in_inf may be NULL (all finite). */
/* The multiplicands must be points of the PRIME-ORDER SUBGROUP -- which every point the g1pubs / g2pubs API can hand to a
 * multiplication is (hash points: Sign; the generators: PrivToPub; keys and signatures that passed Deserialize*'s subgroup
 * check).  For them the multiplication runs through the curve endomorphisms (G1: k = k1 + k2 z^2 with phi; G2: base-|x| digits
 * with psi -- bls_amd/csrc/glv.cuh), half / a quarter of the reference's doublings, the same group element and affine bytes.
 * For ARBITRARY curve points (the reference's bit-serial MulFR accepts any; an on-curve point outside the subgroup fed to the default
 * ladder yields a DIFFERENT point, silently) use the *_ex forms below with BLSMI_MUL_ANY_POINT: the choice is made per call and costs
 * nothing to concurrent callers.  blsmi_set_mul_assume_subgroup(0) / BLSMI_MUL_GENERIC=1 change the PROCESS-WIDE default of the plain
 * entry points instead: every call in flight reads it, so set it once before the first call (legacy switch; prefer the flag). */
#define BLSMI_MUL_ANY_POINT 1u   /* multiplicands may lie outside the prime-order subgroup: plain fixed-window ladder / plain bucket MSM */
int blsmi_set_mul_assume_subgroup(int on);
int blsmi_g1_mul_batch(const uint8_t *pts /* n*96 */, const uint8_t *scalars /* n*32 */, uint8_t *out /* n*96 */, uint8_t *out_inf /* n */, size_t n);
int blsmi_g2_mul_batch(const uint8_t *pts /* n*192 */, const uint8_t *scalars /* n*32 */, uint8_t *out /* n*192 */, uint8_t *out_inf /* n */, size_t n);
/* k_i * generator (PrivToPub g2pubs/bls.go:138-140 uses G2, g1pubs/bls.go:144-146 uses G1).
 * NOT side-channel hardened: the scalar-multiplication kernels index a per-lane table by scalar nibbles and take
 * data-dependent paths in the group law (the reference's bit-serial Mul is not constant-time either); the small-batch
 * level program has a fixed instruction sequence and complete group formulas but still addresses an LDS table by the
 * scalar's digits.  They exist to
 * generate and check test/bench inputs and for public scalars; secret keys belong on the upstream pure-Go module
 * (the one-tuple Sign / PrivToPub stay there in the Go shim). */
int blsmi_g1_mul_generator_batch(const uint8_t *scalars /* n*32 */, uint8_t *out /* n*96 */, uint8_t *out_inf /* n */, size_t n);
int blsmi_g2_mul_generator_batch(const uint8_t *scalars /* n*32 */, uint8_t *out /* n*192 */, uint8_t *out_inf /* n */, size_t n);
/* sum of n points (tree reduction on the device; equals the reference's sequential Jacobian sum
 * after ToAffine).  *out_inf = 1 for the point at infinity. */
int blsmi_g1_sum(const uint8_t *pts, const uint8_t *in_inf, size_t n, uint8_t out[96], int *out_inf);
int blsmi_g2_sum(const uint8_t *pts, const uint8_t *in_inf, size_t n, uint8_t out[192], int *out_inf);
/* multi-scalar multiplication sum_i k_i * P_i (BASELINE config 3; equals summing the reference's MulFR results with
 * AddAssign, compared after ToAffine).  Below 2^17 points: fixed-window multiples + tree sum in one device pass;
 * from there on the bucket method (16-bit windows), with a fallback to the former for degenerate scalar sets. */
int blsmi_g1_msm(const uint8_t *pts /* n*96 */, const uint8_t *scalars /* n*32 */, size_t n, uint8_t out[96], int *out_inf);
int blsmi_g2_msm(const uint8_t *pts /* n*192 */, const uint8_t *scalars /* n*32 */, size_t n, uint8_t out[192], int *out_inf);
/* The same four with the ladder chosen PER CALL: flags = 0 (subgroup points, as above) or BLSMI_MUL_ANY_POINT; other bits: BLSMI_E_ARG. */
int blsmi_g1_mul_batch_ex(const uint8_t *pts, const uint8_t *scalars, uint8_t *out, uint8_t *out_inf, size_t n, unsigned flags);
int blsmi_g2_mul_batch_ex(const uint8_t *pts, const uint8_t *scalars, uint8_t *out, uint8_t *out_inf, size_t n, unsigned flags);
int blsmi_g1_msm_ex(const uint8_t *pts, const uint8_t *scalars, size_t n, uint8_t out[96], int *out_inf, unsigned flags);
int blsmi_g2_msm_ex(const uint8_t *pts, const uint8_t *scalars, size_t n, uint8_t out[192], int *out_inf, unsigned flags);
/* Device-pointer forms of the above (BASELINE config 3 with inputs resident in HBM): every d_* buffer lives on ONE of the
 * library's devices (the call runs on the device that owns d_out), layouts as in the host forms; d_pts == NULL multiplies
 * the group generator; d_out_inf is n bytes, d_in_inf may be NULL.  The single-point results of sum / msm stay on the
 * device (96 / 192 bytes at d_out), their infinity flag comes back through the host int.  `stream` as in
 * blsmi_pairing_batch_dev.  (Added in blsmi 0.3.) */
int blsmi_g1_mul_batch_dev(const void *d_pts, const void *d_scalars, void *d_out, void *d_out_inf, size_t n, void *stream);
int blsmi_g2_mul_batch_dev(const void *d_pts, const void *d_scalars, void *d_out, void *d_out_inf, size_t n, void *stream);
int blsmi_g1_sum_dev(const void *d_pts, const void *d_in_inf, size_t n, void *d_out, int *out_inf, void *stream);
int blsmi_g2_sum_dev(const void *d_pts, const void *d_in_inf, size_t n, void *d_out, int *out_inf, void *stream);
int blsmi_g1_msm_dev(const void *d_pts, const void *d_scalars, size_t n, void *d_out, int *out_inf, void *stream);
int blsmi_g2_msm_dev(const void *d_pts, const void *d_scalars, size_t n, void *d_out, int *out_inf, void *stream);
/* ... and with the per-call ladder choice (flags as for blsmi_g1_mul_batch_ex; d_pts must not be NULL) */
int blsmi_g1_mul_batch_dev_ex(const void *d_pts, const void *d_scalars, void *d_out, void *d_out_inf, size_t n, void *stream, unsigned flags);
int blsmi_g2_mul_batch_dev_ex(const void *d_pts, const void *d_scalars, void *d_out, void *d_out_inf, size_t n, void *stream, unsigned flags);
int blsmi_g1_msm_dev_ex(const void *d_pts, const void *d_scalars, size_t n, void *d_out, int *out_inf, void *stream, unsigned flags);
int blsmi_g2_msm_dev_ex(const void *d_pts, const void *d_scalars, size_t n, void *d_out, int *out_inf, void *stream, unsigned flags);

/* ---- hash to curve (HashG1 hash.go:326-331, HashG2 hash.go:405-411, HashG2WithDomain
 * g2.go:1041-1085) -- messages are concatenated in `msgs`, message i = msgs[off[i] .. off[i+1]) -- */
int blsmi_hash_g1_batch(const uint8_t *msgs, const uint64_t *off /* n+1 */, uint8_t *out /* n*96 */, size_t n);
int blsmi_hash_g2_batch(const uint8_t *msgs, const uint64_t *off /* n+1 */, uint8_t *out /* n*192 */, size_t n);
int blsmi_hash_g2_with_domain_batch(const uint8_t *msgs32 /* n*32 */, const uint8_t domain[8], uint8_t *out /* n*192 */, size_t n);

/* ---- Sign for n (message, secret key) pairs in one call: sig_i = sk_i * H(msg_i) (g2pubs/bls.go:132-135; g1pubs/bls.go:132-135,
 * SignWithDomain :138-141): the hash points stay on the device between the two steps.  sks: n*32 bytes, big-endian scalars (FR as
 * the Go API serialises it); out_inf[i] = 1 when sk_i = 0 mod r (the signature is the point at infinity, written as the all-zero
 * record).  Like the scalar multiplications above these are NOT side-channel hardened, and the secret scalars cross the PCIe bus and
 * live in a device temporary for the duration of the call: bulk signing of test / bench inputs and of keys that may leave the host
 * (the shim's SignBatch); a deployment that must keep its keys in host memory stays on the upstream Sign, and
 * blsmi_prefer_cpu(BLSMI_SHAPE_SIGN, n) says when a small call is faster there anyway. */
int blsmi_g2pubs_sign_batch(const uint8_t *msgs, const uint64_t *off /* n+1 */, const uint8_t *sks /* n*32 */, uint8_t *out_sigs /* n*96 */, uint8_t *out_inf /* n */, size_t n);
int blsmi_g1pubs_sign_batch(const uint8_t *msgs, const uint64_t *off /* n+1 */, const uint8_t *sks /* n*32 */, uint8_t *out_sigs /* n*192 */, uint8_t *out_inf /* n */, size_t n);
int blsmi_g1pubs_sign_with_domain_batch(const uint8_t *msgs32 /* n*32 */, const uint8_t domain[8], const uint8_t *sks /* n*32 */, uint8_t *out_sigs /* n*192 */, uint8_t *out_inf /* n */, size_t n);

/* ---- g2pubs: PublicKey in G2 (192 B affine), Signature in G1 (96 B affine), H: msg -> G1 ------
 * verify_batch: ok[i] = g2pubs.Verify(msg_i, pk_i, sig_i) (g2pubs/bls.go:159-162) as one byte per
 * tuple (0/1) and, if ok_bitmap != NULL, packed LSB-first into ceil(n/8) bytes.
 * inf_flags (may be NULL): bit0 = pk_i is infinity, bit1 = sig_i is infinity -> ok[i] = 0. */
int blsmi_g2pubs_verify_batch(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks /* n*192 */, const uint8_t *sigs /* n*96 */,
                              const uint8_t *inf_flags, uint8_t *ok /* n, may be NULL */, uint8_t *ok_bitmap /* ceil(n/8), may be NULL */, size_t n);
/* (*Signature).VerifyAggregate (g2pubs/bls.go:240-270): one aggregate signature over n (pk_i, msg_i),
 * including the duplicate-message rejection.  *ok = 0/1. */
int blsmi_g2pubs_verify_aggregate(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks, const uint8_t sig[96], size_t n, int *ok);
/* (*Signature).VerifyAggregateCommon (g2pubs/bls.go:275-278) */
int blsmi_g2pubs_verify_aggregate_common(const uint8_t *msg, size_t msg_len, const uint8_t *pks, const uint8_t sig[96], size_t n, int *ok);

/* ---- g1pubs: PublicKey in G1 (96 B), Signature in G2 (192 B), H: msg -> G2 (g1pubs/bls.go) ---- */
int blsmi_g1pubs_verify_batch(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks /* n*96 */, const uint8_t *sigs /* n*192 */,
                              const uint8_t *inf_flags, uint8_t *ok, uint8_t *ok_bitmap, size_t n);
int blsmi_g1pubs_verify_aggregate(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks, const uint8_t sig[192], size_t n, int *ok);
int blsmi_g1pubs_verify_aggregate_common(const uint8_t *msg, size_t msg_len, const uint8_t *pks, const uint8_t sig[192], size_t n, int *ok);
/* the *WithDomain family (g1pubs/bls.go:171-174, 294-311): 32-byte messages, 8-byte domain */
int blsmi_g1pubs_verify_with_domain_batch(const uint8_t *msgs32, const uint8_t domain[8], const uint8_t *pks, const uint8_t *sigs,
                                          const uint8_t *inf_flags, uint8_t *ok, uint8_t *ok_bitmap, size_t n);
int blsmi_g1pubs_verify_aggregate_with_domain(const uint8_t *msgs32, const uint8_t domain[8], const uint8_t *pks, const uint8_t sig[192], size_t n, int *ok);
int blsmi_g1pubs_verify_aggregate_common_with_domain(const uint8_t msg32[32], const uint8_t domain[8], const uint8_t *pks, const uint8_t sig[192], size_t n, int *ok);

/* ---- prepared public keys (g2pubs; added in blsmi 0.4) ---------------------------------------------------------------
 * bls.MillerLoop takes its G2 arguments PREPARED (MillerLoopItem{P *G1Affine, Q *G2Prepared}, pairing.go:4-14;
 * G2AffineToPrepared, g2.go:639-801: the 68 line-coefficient triples that depend on Q alone), and g2pubs.Verify prepares the
 * same public key again on every call (CompareTwoPairings, pairing.go:140-147).  A verifier that meets the same keys again and
 * again prepares them ONCE into device memory -- BLSMI_G2_PREPARED_BYTES per key, one table after the other -- and hands the
 * tables to the *_prepared_dev entry points, whose Miller loops read a key's lines instead of recomputing them.
 * d_key_idx: n x uint32, tuple t uses table d_key_idx[t]; NULL: tuple t uses table t.  Indices are NOT range-checked (the tables
 * are plain memory the caller sized): an index beyond the prepared keys reads past them.  A key given as the all-zero record
 * (the point at infinity) keeps that mark in its table: verdict 0, as in the unprepared forms.  Every result is identical to the
 * unprepared entry point on the same keys.  All buffers on ONE of the library's devices; `stream` as in blsmi_pairing_batch_dev. */
#define BLSMI_G2_PREPARED_BYTES 24704
int blsmi_g2_prepare_batch_dev(const void *d_g2_aff /* n*192 */, size_t n, void *d_prepared /* n*BLSMI_G2_PREPARED_BYTES */, void *stream);
/* the reference's G2Prepared.coeffs of n prepared keys: per key 68 x [3]FQ2, each FQ2 as c0 | c1, 6 x uint64 Montgomery limbs each */
int blsmi_g2_prepared_export_dev(const void *d_prepared, size_t n, void *d_out /* n*68*3*12 uint64 */, void *stream);
/* G2AffineToPrepared of n host points straight into that representation (BenchmarkG2Prepare, pairing_test.go:60-81) */
int blsmi_g2_prepare_batch(const uint8_t *g2_aff /* n*192 */, size_t n, uint64_t *out_coeffs /* n*68*3*12 */);
/* For callers without a HIP runtime of their own (the cgo shim): prepare n HOST keys into tables the library allocates on one of
 * its devices; *handle is the device pointer to pass as d_prepared.  _destroy waits for that device to go idle, then frees. */
int blsmi_g2_prepared_create(const uint8_t *g2_aff /* n*192 */, size_t n, void **handle);
int blsmi_g2_prepared_destroy(void *handle);
/* n independent g2pubs.Verify()s with messages, signatures, key indices and results in HOST memory and the keys prepared;
 * arguments as blsmi_g2pubs_verify_batch with (d_prepared, key_idx) in the place of pks.  Runs on the device that holds the
 * tables (not split over devices). */
int blsmi_g2pubs_verify_batch_prepared(const uint8_t *msgs, const uint64_t *msg_off, const void *d_prepared, const uint32_t *key_idx /* n, may be NULL */,
                                       const uint8_t *sigs, const uint8_t *inf_flags, uint8_t *ok, uint8_t *ok_bitmap, size_t n);
/* Pairing(P_t, Q_t) with Q_t prepared; output as blsmi_pairing_batch_dev */
int blsmi_pairing_batch_prepared_dev(const void *d_g1_aff, const void *d_prepared, const void *d_key_idx, void *d_out_fq12, size_t n, void *stream);
/* g2pubs.Verify x n / Signature.VerifyAggregate with prepared public keys; otherwise as the *_dev forms below */
int blsmi_g2pubs_verify_batch_prepared_dev(const void *d_msgs, const void *d_off, const void *d_prepared, const void *d_key_idx,
                                           const void *d_sigs, const void *d_inf_flags, void *d_ok, size_t n, void *stream);
int blsmi_g2pubs_verify_aggregate_prepared(const uint8_t *msgs, const uint64_t *msg_off, const void *d_prepared, const uint32_t *key_idx /* n, may be NULL */,
                                           const uint8_t sig[96], size_t n, int *ok);   /* messages, indices and signature in HOST memory */
int blsmi_g2pubs_verify_aggregate_prepared_dev(const void *d_msgs, const void *d_off, const void *d_prepared, const void *d_key_idx,
                                               const uint8_t sig[96], size_t n, int *ok, void *stream);

/* ---- the reference's in-memory points at the boundary (added in blsmi 0.6) ---------------------------------------------------
 * The Go types hold their points in Jacobian coordinates and Montgomery limbs: Signature{s *bls.G1Projective}, PublicKey{p *bls.G2Projective}
 * (g2pubs/bls.go:13-15, 53-55; swapped in g1pubs), G1Projective{x, y, z FQ} (g1.go:252-256), G2Projective{x, y, z FQ2} (g2.go:298-302),
 * FQ2{c0, c1 FQ} (fq2.go:14-17), FQ{n FQRepr} (fq.go:11-13), FQRepr [6]uint64 little-endian (fqrepr.go:14), Montgomery form R = 2^384.  The
 * affine entry points above make the shim run ToAffine() -- one Fq inversion per point, g1.go:322-340 -- and SerializeBytes() -- two MontReduce
 * and a byte swap, g1.go:157-167 -- on a host core for every point: ~12 us each, 30-70x the device's cost of the whole verify.  The *_jac
 * forms take the struct bytes AS THEY LIE:
 *     G1 point = 18 x uint64 (x | y | z),            BLSMI_G1_JAC_BYTES = 144
 *     G2 point = 36 x uint64 (x.c0 | x.c1 | y.c0 | y.c1 | z.c0 | z.c1), BLSMI_G2_JAC_BYTES = 288
 * i.e. *(*[18]uint64)(unsafe.Pointer(sig.s)) -- one memcpy per point in the shim, nothing else -- and run ToAffine on the device (a wave
 * whose 64 points all have z == 1, what Deserialize* leaves, skips the inversion like g2.go:368).  z == 0 is the point at infinity
 * (G1Projective.IsZero g1.go:287-289): such a tuple gets verdict 0, so there are no inf_flags here.  The reference's arithmetic keeps every
 * FQ below q (fq.go:37-45); a limb image that is NOT below q cannot come out of it and is read as 0, the way FQReprToFQ reads an invalid
 * repr (fq.go:49-56).  Results are identical, bit for bit, to the affine entry points on ToAffine().SerializeBytes() of the same points.
 * Arguments other than the points are as in the affine forms. */
#define BLSMI_G1_JAC_BYTES 144
#define BLSMI_G2_JAC_BYTES 288
/* G?Projective.ToAffine().SerializeBytes() for n points: wire records (all zero for infinity), out_inf[i] = 1 for infinity (may be NULL) */
int blsmi_g1_jac_to_affine_batch(const uint64_t *g1_jac /* n*18 */, uint8_t *out /* n*96 */, uint8_t *out_inf /* n */, size_t n);
int blsmi_g2_jac_to_affine_batch(const uint64_t *g2_jac /* n*36 */, uint8_t *out /* n*192 */, uint8_t *out_inf /* n */, size_t n);
/* bls.Pairing(p *G1Projective, q *G2Projective) (pairing.go:132-136) for n pairs; output as blsmi_pairing_batch */
int blsmi_pairing_batch_jac(const uint64_t *g1_jac /* n*18 */, const uint64_t *g2_jac /* n*36 */, uint64_t *out_fq12 /* n*72 */, size_t n);
/* AggregateSignatures / AggregatePublicKeys (g2pubs/bls.go:165-192): the sum of n in-memory points, handed back as an in-memory point with
 * z = 1 -- (0, 1, 0), the reference's G?ProjectiveZero, for the point at infinity (*out_inf = 1; also for n = 0).  The points are added
 * as they are (Jacobian + Jacobian, g1.go:400-470): no inversion but the one at the end. */
int blsmi_g1_sum_jac(const uint64_t *g1_jac /* n*18 */, size_t n, uint64_t out_jac[18], int *out_inf);
int blsmi_g2_sum_jac(const uint64_t *g2_jac /* n*36 */, size_t n, uint64_t out_jac[36], int *out_inf);
/* Results in the in-memory form: PrivToPub (k_i * generator) and Sign (sk_i * H(m_i)) for n scalars, each result a bls.G?Projective record with
 * z = 1 -- (0, 1, 0) when the scalar is 0 mod r -- so that the shim builds its PublicKey / Signature by one copy (upstream: FQReprToFQ per coordinate).
 * Same caveats as the affine forms (not side-channel hardened; secret scalars cross the bus). */
int blsmi_g1_mul_generator_batch_jac(const uint8_t *scalars /* n*32 */, uint64_t *out_jac /* n*18 */, size_t n);
int blsmi_g2_mul_generator_batch_jac(const uint8_t *scalars /* n*32 */, uint64_t *out_jac /* n*36 */, size_t n);
int blsmi_g2pubs_sign_batch_jac(const uint8_t *msgs, const uint64_t *off /* n+1 */, const uint8_t *sks /* n*32 */, uint64_t *out_sigs_jac /* n*18 */, size_t n);
int blsmi_g1pubs_sign_batch_jac(const uint8_t *msgs, const uint64_t *off /* n+1 */, const uint8_t *sks /* n*32 */, uint64_t *out_sigs_jac /* n*36 */, size_t n);
int blsmi_g1pubs_sign_with_domain_batch_jac(const uint8_t *msgs32 /* n*32 */, const uint8_t domain[8], const uint8_t *sks /* n*32 */, uint64_t *out_sigs_jac /* n*36 */, size_t n);
/* g2pubs (PublicKey = G2Projective 36 x u64, Signature = G1Projective 18 x u64) */
int blsmi_g2pubs_verify_batch_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*36 */, const uint64_t *sigs /* n*18 */,
                                  uint8_t *ok /* n, may be NULL */, uint8_t *ok_bitmap /* ceil(n/8), may be NULL */, size_t n);
int blsmi_g2pubs_verify_aggregate_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*36 */, const uint64_t sig[18], size_t n, int *ok);
int blsmi_g2pubs_verify_aggregate_common_jac(const uint8_t *msg, size_t msg_len, const uint64_t *pks /* n*36 */, const uint64_t sig[18], size_t n, int *ok);
/* g1pubs (PublicKey = G1Projective 18 x u64, Signature = G2Projective 36 x u64) */
int blsmi_g1pubs_verify_batch_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                  uint8_t *ok, uint8_t *ok_bitmap, size_t n);
int blsmi_g1pubs_verify_with_domain_batch_jac(const uint8_t *msgs32, const uint8_t domain[8], const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                              uint8_t *ok, uint8_t *ok_bitmap, size_t n);
int blsmi_g1pubs_verify_aggregate_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*18 */, const uint64_t sig[36], size_t n, int *ok);
int blsmi_g1pubs_verify_aggregate_with_domain_jac(const uint8_t *msgs32, const uint8_t domain[8], const uint64_t *pks /* n*18 */, const uint64_t sig[36], size_t n, int *ok);
int blsmi_g1pubs_verify_aggregate_common_jac(const uint8_t *msg, size_t msg_len, const uint64_t *pks /* n*18 */, const uint64_t sig[36], size_t n, int *ok);
int blsmi_g1pubs_verify_aggregate_common_with_domain_jac(const uint8_t msg32[32], const uint8_t domain[8], const uint64_t *pks /* n*18 */, const uint64_t sig[36], size_t n, int *ok);
/* ---- randomised batch verification (blsmi 0.8) ------------------------------------------------------------------------------
 * One pairing check per batch (small-exponent batch verification, Bellare-Garay-Rabin 1998): with random nonzero 64-bit r_i,
 *     g2pubs: e(sum r_i sig_i, G2gen) == prod e(r_i H(m_i), pk_i)        g1pubs: e(G1gen, sum r_i sig_i) == prod e(r_i pk_i, H(m_i))
 * n Miller loops, a product tree and ONE final exponentiation instead of 2n Miller loops and n final exponentiations.
 * Same arguments and results as the verify_batch entry point each mirrors, plus `scalars` and `combined`:
 *   - combined check holds: ok[i] = 1 for every tuple, none checked on its own.  Every invalid tuple among them makes it hold with
 *     probability at most 2^-64 over the r_i.
 *   - it fails: the per-tuple verdicts of verify_batch, computed from the inputs already on the device (the failing call costs about a
 *     verify_batch on top of the combined check).  Bisection is not attempted.  (blsmi 0.12: *_verify_batch_rlc_locate below rechecks by blocks.)
 *   - a key or signature at infinity (inf_flags, the all-zero record, or z = 0 in the in-memory forms) gets ok[i] = 0 as in verify_batch;
 *     any point at infinity on the combined path (an input, a scaled r_i H_i / r_i pk_i, the sum) sends the call (or its shard) to the
 *     per-tuple path.
 *   - scalars (n, may be NULL): NULL draws n fresh nonzero 64-bit scalars per call from the OS (getrandom(2), else /dev/urandom;
 *     BLSMI_E_RNG when neither works).  Caller scalars: a zero among them is BLSMI_E_ARG, and the soundness of the check is then the
 *     CALLER's responsibility (the scalars must be unpredictable to whoever made the signatures); they exist so that tests can pin the arithmetic.
 *   - combined (may be NULL): 1 when every verdict came from a combined check that held; 0 when the call, or any shard of a split call,
 *     took the per-tuple path (the check failed, a point at infinity, fewer than "rlc_min" tuples) and for n = 0.
 * PRECONDITION: soundness is stated for keys and signatures in the prime-order subgroups -- what Deserialize guarantees (g1.go:185-197,
 * g2.go:219-230).  The arithmetic itself (a plain 64-bit ladder, the any-point bucket MSM) is exact for any curve point.
 * Below blsmi_set_option("rlc_min", n) / BLSMI_RLC_MIN tuples the per-tuple path runs directly (combined = 0).  These calls never join
 * the request combiner of verify_batch; a large call is split over the devices like verify_batch, one combined check per shard. */
int blsmi_g2pubs_verify_batch_rlc(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks /* n*192 */, const uint8_t *sigs /* n*96 */, const uint8_t *inf_flags,
                                  const uint64_t *scalars /* n, may be NULL */, uint8_t *ok /* n, may be NULL */, uint8_t *ok_bitmap /* may be NULL */, size_t n, int *combined);
int blsmi_g1pubs_verify_batch_rlc(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks /* n*96 */, const uint8_t *sigs /* n*192 */, const uint8_t *inf_flags,
                                  const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g1pubs_verify_with_domain_batch_rlc(const uint8_t *msgs32, const uint8_t domain[8], const uint8_t *pks, const uint8_t *sigs, const uint8_t *inf_flags,
                                              const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
/* in-memory forms (the shims' VerifyBatchRandomized), shaped like blsmi_g?pubs_verify_batch_jac */
int blsmi_g2pubs_verify_batch_rlc_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*36 */, const uint64_t *sigs /* n*18 */,
                                      const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g1pubs_verify_batch_rlc_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                      const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g1pubs_verify_with_domain_batch_rlc_jac(const uint8_t *msgs32, const uint8_t domain[8], const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                                  const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
/* ---- grouped randomised batch verification (blsmi 0.11) ---------------------------------------------------------------------
 * The combined check above for batches whose tuples share messages (an attestation subnet, a slot, a sync committee: thousands of
 * signatures over a few dozen messages).  The messages are a table of d entries -- msgs with msg_off[d + 1] (with_domain: msgs32, d * 32
 * bytes) -- and tuple i is (msgs[msg_idx[i]], pk_i, sig_i).  Bilinearity lets the tuples of one message share one pairing:
 *     g1pubs: e(G1gen, sum_i r_i sig_i) == prod_g e(sum_{i in g} r_i pk_i, H(m_g))
 *     g2pubs: e(sum_i r_i sig_i, G2gen) == prod_g e(H(m_g), sum_{i in g} r_i pk_i)
 * d' hashes and d' Miller loops for the d' table entries some tuple refers to, not n; the signature side is that of *_verify_batch_rlc.
 * ok, ok_bitmap, inf_flags, scalars and combined mean exactly what they mean there, and the verdicts are those of *_verify_batch_rlc (and
 * so of *_verify_batch) on the expanded messages.  The weights are per TUPLE also inside a group: with caller scalars r_a == r_b two tuples
 * of one message may swap signatures unnoticed -- the caller's responsibility, as every caller scalar is.
 *   - msg_idx[i] >= d (d = 0 with n > 0 included), a zero caller scalar, and a NULL input with n > 0: BLSMI_E_ARG before any device work.
 *     n = 0: BLSMI_OK, combined = 0.
 *   - table entries with equal bytes are not merged (the result is correct, the call shares less); entries no tuple refers to are never hashed.
 *   - the per-tuple path (combined = 0) runs when the check fails and when a point at infinity meets it: an input (inf_flags, the all-zero
 *     record, z = 0 in the in-memory forms), a group whose weighted sum is infinity, the signatures' sum.
 * "rlc_min" does NOT apply: calling this form is the caller's choice of the combined path, at any n.  The call runs on one device (it is not
 * split like *_verify_batch_rlc) and never joins the request combiner, like the pairing products.
 * When to call it (one MI355X, host buffers, ms; profiles/r08_rlc_grouped.log; rlc / batch = *_verify_batch_rlc at rlc_min = 0 and
 * *_verify_batch of the build before this form, messages expanded):
 *     n x d              g2pubs grouped / rlc / batch      g1pubs grouped / rlc / batch
 *     1 024 x 64              8.0 /  5.9 /  2.7                 8.4 /  8.3 /  3.4
 *     16 384 x 64            10.1 / 11.0 /  8.7                12.5 / 16.2 / 10.6
 *     65 536 x 64            13.3 / 17.5 / 27.2                14.6 / 25.0 / 32.1
 *     65 536 x 8 192         18.5 / 17.5 / 27.2                18.0 / 25.1 / 32.1
 *     65 536 x 65 536        59.2 / 17.4 / 26.4                43.5 / 25.2 / 32.1
 * It pays from some tens of thousands of tuples with d up to a few thousand (1.3x / 1.7x the plain randomised form at 65 536 x 64); the call has
 * a floor of about 8 ms, and with d near n it loses badly (one final pass and one cleared hash per message): call *_verify_batch_rlc there.  One
 * bad tuple at 65 536 x 64 costs 36.8 / 40.6 ms (the combined check, then the per-tuple path). */
int blsmi_g2pubs_verify_batch_rlc_grouped(const uint8_t *msgs, const uint64_t *msg_off /* d+1 */, size_t d, const uint32_t *msg_idx /* n */,
                                          const uint8_t *pks /* n*192 */, const uint8_t *sigs /* n*96 */, const uint8_t *inf_flags,
                                          const uint64_t *scalars /* n, may be NULL */, uint8_t *ok /* n, may be NULL */, uint8_t *ok_bitmap /* may be NULL */, size_t n, int *combined);
int blsmi_g1pubs_verify_batch_rlc_grouped(const uint8_t *msgs, const uint64_t *msg_off /* d+1 */, size_t d, const uint32_t *msg_idx /* n */,
                                          const uint8_t *pks /* n*96 */, const uint8_t *sigs /* n*192 */, const uint8_t *inf_flags,
                                          const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped(const uint8_t *msgs32 /* d*32 */, const uint8_t domain[8], size_t d, const uint32_t *msg_idx /* n */,
                                                      const uint8_t *pks, const uint8_t *sigs, const uint8_t *inf_flags,
                                                      const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g2pubs_verify_batch_rlc_grouped_jac(const uint8_t *msgs, const uint64_t *msg_off, size_t d, const uint32_t *msg_idx, const uint64_t *pks /* n*36 */, const uint64_t *sigs /* n*18 */,
                                              const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g1pubs_verify_batch_rlc_grouped_jac(const uint8_t *msgs, const uint64_t *msg_off, size_t d, const uint32_t *msg_idx, const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                              const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac(const uint8_t *msgs32, const uint8_t domain[8], size_t d, const uint32_t *msg_idx, const uint64_t *pks /* n*18 */,
                                                          const uint64_t *sigs /* n*36 */, const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined);
/* ---- randomised batch verification that finds the bad tuples by blocks (blsmi 0.12) ------------------------------------------
 * *_verify_batch_rlc for input an adversary may have touched.  There one invalid tuple sends all n through the per-tuple path; here the
 * batch is cut into contiguous blocks of `block` tuples (the last one may be shorter) and the call keeps every block's product of
 * Miller values.  The total check is that of *_verify_batch_rlc.  When it fails, one pairing equation per block --
 *     g2pubs: e(S_b, G2gen) == prod_{i in b} e(r_i H(m_i), pk_i)      g1pubs: e(G1gen, S_b) == prod_{i in b} e(r_i pk_i, H(m_i))      S_b = sum_{i in b} r_i sig_i
 * -- decides which blocks hold, and the tuples of the blocks that fail, and only those, get the per-tuple verdicts of *_verify_batch.
 * ok[i] = 1 for every tuple of a block whose equation held: its weights are its own tuples' r_i, so such a block is wrong with probability
 * at most 2^-64, as the whole batch is above.  ok, ok_bitmap, inf_flags and scalars mean what they mean there, with the same soundness
 * statement and precondition (caller scalars r_a == r_c let two tuples OF ONE BLOCK carry sig_a + D and sig_c - D unnoticed).
 *   - block: 0 = automatic, the next even number >= max(64, ceil(n / 256)).  Any other value must be even and at least 2 (two consecutive
 *     tuples share one Miller loop in the layouts of large calls, so a block border must be a border there too); block >= n gives one block.
 *   - an odd block or block = 1, a zero caller scalar, and a NULL input with n > 0: BLSMI_E_ARG before any device work.  n = 0: BLSMI_OK,
 *     combined = 0, rechecked = 0.
 *   - combined (may be NULL): 1 exactly when the total check held (every verdict is 1 then); 0 otherwise and for n = 0.
 *   - rechecked (may be NULL): the number of tuples whose verdict came from the per-tuple path -- 0 when the total check held, the sum of the
 *     sizes of the failing blocks otherwise.
 *   - a block fails, whatever its equation says, when one of its tuples is at infinity (inf_flags, the all-zero record, z = 0 in the in-memory
 *     forms, a scaled r_i H_i / r_i pk_i) or its S_b is; with such a tuple anywhere, or sum r_i sig_i at infinity, the total's verdict is not
 *     consulted and the block checks run.
 * "rlc_min" does NOT apply, the call runs on one device and never joins the request combiner, as the grouped form.  The hash points are
 * always cleared of their cofactor here (from 65 536 messages g2pubs' *_verify_batch_rlc clears the product instead).
 * When to call it (one MI355X, host buffers, ms, median of 10; profiles/r09_rlc_locate.log; rlc / batch = *_verify_batch_rlc at rlc_min = 0
 * and *_verify_batch of the build before this form):
 *     n, bad tuples          g2pubs locate / rlc / batch      g1pubs locate / rlc / batch
 *     16 384, none               11.0 / 11.0 /  8.7                16.3 / 16.4 / 10.7
 *     16 384, one                16.2 / 18.3 /  8.4                23.7 / 24.0 / 10.2
 *     65 536, none               17.6 / 17.3 / 26.9                24.9 / 25.0 / 31.6
 *     65 536, one                23.8 / 42.7 / 25.2                34.6 / 50.5 / 30.2
 *     65 536, 16 in 16 blocks    25.0 / 42.6 / 25.2                36.2 / 50.4 / 30.1
 * The call that holds costs what *_verify_batch_rlc costs (the differences are inside the run-to-run spread of 0.3 .. 0.7 ms, g2pubs at 65 536 with
 * its cleared hash included).  A failing call costs the block checks on top -- about 6 ms (g2pubs) / 10 ms (g1pubs) at 65 536: the n 64-bit
 * multiples of the block sums, 256 Miller loops and final exponentiations -- plus the failing blocks' tuples: call it wherever *_verify_batch_rlc pays and the input is not trusted.  Below
 * some tens of thousands of tuples *_verify_batch is the faster call, as for *_verify_batch_rlc. */
int blsmi_g2pubs_verify_batch_rlc_locate(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks /* n*192 */, const uint8_t *sigs /* n*96 */, const uint8_t *inf_flags,
                                         const uint64_t *scalars /* n, may be NULL */, size_t block, uint8_t *ok /* n, may be NULL */, uint8_t *ok_bitmap /* may be NULL */, size_t n,
                                         int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_batch_rlc_locate(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks /* n*96 */, const uint8_t *sigs /* n*192 */, const uint8_t *inf_flags,
                                         const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_with_domain_batch_rlc_locate(const uint8_t *msgs32, const uint8_t domain[8], const uint8_t *pks, const uint8_t *sigs, const uint8_t *inf_flags,
                                                     const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
int blsmi_g2pubs_verify_batch_rlc_locate_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*36 */, const uint64_t *sigs /* n*18 */,
                                             const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_batch_rlc_locate_jac(const uint8_t *msgs, const uint64_t *off, const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                             const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac(const uint8_t *msgs32, const uint8_t domain[8], const uint64_t *pks /* n*18 */, const uint64_t *sigs /* n*36 */,
                                                         const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
/* ---- grouped randomised batch verification that finds the bad tuples by cells (blsmi 0.13) -----------------------------------
 * *_verify_batch_rlc_grouped for input an adversary may have touched: the batches that share messages (a subnet, a slot, a sync
 * committee) are the ones anybody can put a bad signature into, and there one invalid tuple sends all n through the per-tuple path.  The
 * arguments are those of *_verify_batch_rlc_grouped with `block` after `scalars` and `rechecked` at the end, as in *_verify_batch_rlc_locate;
 * ok, ok_bitmap, inf_flags, scalars and combined mean what they mean in the grouped form, rechecked what it means in the block-locating
 * form, and the verdicts are those of *_verify_batch on the expanded messages.
 * The tuples are sorted by message (stable: the tuples of one message keep their input order), and every message's tuples are cut, in that
 * order, into CELLS of at most `block` consecutive tuples: in each group every cell but the last is full, and no cell crosses a group
 * border.  The call sums keys AND signatures per cell -- K_c = sum_{i in c} r_i pk_i, S_c = sum_{i in c} r_i sig_i -- runs one Miller loop
 * per cell and keeps its value; the total check is the grouped form's, its two sides being the product of the cell values and the sum of
 * the S_c.  When it fails, one pairing equation per cell decides, from what is already on the device (nothing is scaled again) --
 *     g2pubs: e(S_c, G2gen) == e(H(m_g(c)), K_c)        g1pubs: e(G1gen, S_c) == e(K_c, H(m_g(c)))
 * -- and the tuples of the cells that fail, and only those, get the per-tuple verdicts of *_verify_batch.  A cell's weights are its own
 * tuples' r_i, so a cell whose equation holds is wrong with probability at most 2^-64, as the whole batch is.  With caller scalars
 * r_a == r_c two tuples OF ONE CELL may carry sig_a + D and sig_c - D unnoticed, and two tuples of one group may swap signatures (the
 * grouped form's caveat) -- the caller's responsibility, as every caller scalar is.  The subgroup precondition of *_verify_batch_rlc applies.
 *   - block: 0 = automatic, the rule of *_verify_batch_rlc_locate (the next even number >= max(64, ceil(n / 256))).  Any other value >= 1 is
 *     accepted; there is no evenness rule here, each cell has a Miller loop of its own.  block >= the largest group makes cells equal to
 *     groups: the call then locates by message.
 *   - msg_idx[i] >= d (d = 0 with n > 0 included), a zero caller scalar, a NULL input with n > 0, and n > 2^32 - 1: BLSMI_E_ARG before any
 *     device work.  n = 0: BLSMI_OK, combined = 0, rechecked = 0.
 *   - combined (may be NULL): 1 exactly when the total check held (every verdict is 1 then); 0 otherwise and for n = 0.
 *   - rechecked (may be NULL): the number of tuples whose verdict came from the per-tuple path -- 0 when the total check held, the sum of the
 *     sizes of the failing cells otherwise.
 *   - a cell fails, whatever its equation says, when one of its tuples is at infinity (inf_flags, the all-zero record, z = 0 in the
 *     in-memory forms), its K_c is, or its S_c is; with such a tuple or K_c anywhere, or sum r_i sig_i at infinity, the total's verdict is
 *     not consulted and the cell checks run.
 * "rlc_min" does NOT apply, the call runs on one device and never joins the request combiner, as the grouped form.  The hash points are
 * always cleared of their cofactor.
 * When to call it (one MI355X, host buffers, ms, median of 10; profiles/r10_rlc_grouped_locate.log; grouped / batch =
 * *_verify_batch_rlc_grouped and *_verify_batch, messages expanded, of the build before this form, on the same tuples):
 *     n x d, bad tuples          g2pubs cells / grouped / batch      g1pubs cells / grouped / batch
 *     16 384 x 64, none                6.8 / 10.1 /  8.5                  7.7 / 12.4 / 10.4
 *     16 384 x 64, one                10.3 / 17.3 /  8.2                 11.2 / 20.1 /  9.9
 *     65 536 x 64, none               11.9 / 13.3 / 25.3                 12.6 / 14.6 / 31.1
 *     65 536 x 64, one                15.5 / 36.0 / 24.4                 16.2 / 39.7 / 29.7
 *     65 536 x 64, 16 in 16 cells     16.6 / 36.1 / 24.6                 17.8 / 39.8 / 29.7
 *     65 536 x 8 192, none            18.5 / 18.7 / 25.4                 20.6 / 18.1 / 31.0
 * (spreads, max - min of the ten, 0.05 .. 0.8 ms.)  With one bad tuple at 65 536 x 64 the call costs 0.43x / 0.41x the grouped form's failing call and
 * stays below *_verify_batch; a failing call pays about 3.6 ms over the call that holds -- 256 Miller loops and final exponentiations and
 * the 256 rechecked tuples, no sum is taken again.  The call that holds is not slower than the grouped form where messages are shared widely
 * (-1.4 / -2.1 ms at 65 536 x 64, -3.2 / -4.8 ms at 16 384 x 64: the signatures' segmented sum is enqueued whole, the MSM it replaces waits on
 * the host between its passes); with few tuples per message it is level (g2pubs) or slower (g1pubs +2.5 ms at 65 536 x 8 192: 8 192 cells, a
 * Miller loop and a final pass of the G2 sums each): call *_verify_batch_rlc_locate or *_verify_batch_rlc_grouped there.  At 16 384 x 64 one
 * bad tuple still leaves *_verify_batch the faster call (8.2 / 9.9 ms). */
int blsmi_g2pubs_verify_batch_rlc_grouped_locate(const uint8_t *msgs, const uint64_t *msg_off /* d+1 */, size_t d, const uint32_t *msg_idx /* n */,
                                                 const uint8_t *pks /* n*192 */, const uint8_t *sigs /* n*96 */, const uint8_t *inf_flags,
                                                 const uint64_t *scalars /* n, may be NULL */, size_t block, uint8_t *ok /* n, may be NULL */, uint8_t *ok_bitmap /* may be NULL */,
                                                 size_t n, int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_batch_rlc_grouped_locate(const uint8_t *msgs, const uint64_t *msg_off /* d+1 */, size_t d, const uint32_t *msg_idx /* n */,
                                                 const uint8_t *pks /* n*96 */, const uint8_t *sigs /* n*192 */, const uint8_t *inf_flags,
                                                 const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate(const uint8_t *msgs32 /* d*32 */, const uint8_t domain[8], size_t d, const uint32_t *msg_idx /* n */,
                                                             const uint8_t *pks, const uint8_t *sigs, const uint8_t *inf_flags,
                                                             const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n, int *combined, size_t *rechecked);
int blsmi_g2pubs_verify_batch_rlc_grouped_locate_jac(const uint8_t *msgs, const uint64_t *msg_off, size_t d, const uint32_t *msg_idx, const uint64_t *pks /* n*36 */,
                                                     const uint64_t *sigs /* n*18 */, const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n,
                                                     int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac(const uint8_t *msgs, const uint64_t *msg_off, size_t d, const uint32_t *msg_idx, const uint64_t *pks /* n*18 */,
                                                     const uint64_t *sigs /* n*36 */, const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n,
                                                     int *combined, size_t *rechecked);
int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(const uint8_t *msgs32, const uint8_t domain[8], size_t d, const uint32_t *msg_idx, const uint64_t *pks /* n*18 */,
                                                                 const uint64_t *sigs /* n*36 */, const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *ok_bitmap, size_t n,
                                                                 int *combined, size_t *rechecked);
/* device-pointer forms (every buffer on ONE of the library's devices; `stream` as in blsmi_pairing_batch_dev): the points resident in HBM as the
 * Go side holds them.  d_ok: n verdict bytes on the device. */
int blsmi_pairing_batch_jac_dev(const void *d_g1_jac, const void *d_g2_jac, void *d_out_fq12, size_t n, void *stream);
int blsmi_g2pubs_verify_batch_jac_dev(const void *d_msgs, const void *d_off, const void *d_pks_jac, const void *d_sigs_jac, void *d_ok, size_t n, void *stream);
int blsmi_g1pubs_verify_batch_jac_dev(const void *d_msgs, const void *d_off, const void *d_pks_jac, const void *d_sigs_jac, void *d_ok, size_t n, void *stream);
int blsmi_g1pubs_verify_with_domain_batch_jac_dev(const void *d_msgs32, const void *d_domain8, const void *d_pks_jac, const void *d_sigs_jac, void *d_ok, size_t n, void *stream);
/* prepared keys (see above) made from, and verified against, in-memory points */
int blsmi_g2_prepared_create_jac(const uint64_t *g2_jac /* n*36 */, size_t n, void **handle);
int blsmi_g2pubs_verify_batch_prepared_jac(const uint8_t *msgs, const uint64_t *msg_off, const void *d_prepared, const uint32_t *key_idx /* n, may be NULL */,
                                           const uint64_t *sigs /* n*18 */, uint8_t *ok, uint8_t *ok_bitmap, size_t n);
int blsmi_g2pubs_verify_aggregate_prepared_jac(const uint8_t *msgs, const uint64_t *msg_off, const void *d_prepared, const uint32_t *key_idx /* n, may be NULL */,
                                               const uint64_t sig[18], size_t n, int *ok);

/* Multi-GPU VerifyAggregate: each rank computes the product of its shard's Miller loops
 * prod_i ML(H(m_i), pk_i) (no final exponentiation) as one Fq12 in the wire format; the ranks all-gather
 * the 576-byte partials, multiply them (blsmi_fq12_product) and finish with one final exponentiation.  The value is
 * meaningful only under that final exponentiation: it is a Miller value of the product, not a fixed representative
 * (projective line functions; from 65 536 messages a g2pubs shard pairs its hash points before their cofactor clearing
 * and raises its product to the cofactor multiplier instead). */
int blsmi_g2pubs_aggregate_partial(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks, size_t n, uint64_t *out_fq12 /* 72 */, int *bad /* may be NULL: 1 if a key is infinity */);
int blsmi_g1pubs_aggregate_partial(const uint8_t *msgs, const uint64_t *off, const uint8_t *pks, size_t n, uint64_t *out_fq12 /* 72 */, int *bad);
int blsmi_fq12_product(const uint64_t *in_fq12 /* n*72 */, size_t n, uint64_t *out_fq12 /* 72 */);

/* device-pointer forms of the verify batches (inputs resident in HBM; ok is n bytes on the device) */
int blsmi_g2pubs_verify_batch_dev(const void *d_msgs, const void *d_off, const void *d_pks, const void *d_sigs, const void *d_inf_flags, void *d_ok, size_t n, void *stream);
int blsmi_g1pubs_verify_batch_dev(const void *d_msgs, const void *d_off, const void *d_pks, const void *d_sigs, const void *d_inf_flags, void *d_ok, size_t n, void *stream);
/* VerifyWithDomain (g1pubs/bls.go:171-174): n 32-byte messages and the 8-byte domain resident on the device */
int blsmi_g1pubs_verify_with_domain_batch_dev(const void *d_msgs32, const void *d_domain8, const void *d_pks, const void *d_sigs, const void *d_inf_flags, void *d_ok, size_t n, void *stream);

/* device-pointer forms of VerifyAggregate (g2pubs/bls.go:240-270, g1pubs/bls.go:252-282, :300-311): messages, offsets (or the
 * 8-byte domain) and keys resident on one of the library's devices, the aggregate signature in HOST memory (one point).  The
 * duplicate-message rejection runs on the device as well (a keyed open-addressing table; every occupied slot of a probe sequence is
 * compared exactly).
 * The call runs on the device that owns d_pks and is not split over devices.  (Added in blsmi 0.3.) */
int blsmi_g2pubs_verify_aggregate_dev(const void *d_msgs, const void *d_off, const void *d_pks, const uint8_t sig[96], size_t n, int *ok, void *stream);
int blsmi_g1pubs_verify_aggregate_dev(const void *d_msgs, const void *d_off, const void *d_pks, const uint8_t sig[192], size_t n, int *ok, void *stream);
int blsmi_g1pubs_verify_aggregate_with_domain_dev(const void *d_msgs32, const void *d_domain, const void *d_pks, const uint8_t sig[192], size_t n, int *ok, void *stream);

/* device-pointer forms of VerifyAggregateCommon (g2pubs/bls.go:275-278, g1pubs/bls.go:287-297): the n public keys resident on one of
 * the library's devices (a validator set kept in HBM) are summed where they lie, then one Verify runs; message, domain and signature are
 * HOST bytes.  n = 0: the empty sum is the point at infinity, verdict 0.  (blsmi 0.5) */
int blsmi_g2pubs_verify_aggregate_common_dev(const void *d_pks /* n*192 */, size_t n, const uint8_t *msg, size_t msg_len, const uint8_t sig[96], int *ok, void *stream);
int blsmi_g1pubs_verify_aggregate_common_dev(const void *d_pks /* n*96 */, size_t n, const uint8_t *msg, size_t msg_len, const uint8_t sig[192], int *ok, void *stream);
int blsmi_g1pubs_verify_aggregate_common_with_domain_dev(const void *d_pks /* n*96 */, size_t n, const uint8_t msg32[32], const uint8_t domain[8], const uint8_t sig[192], int *ok, void *stream);

/* ---- Deserialize + Verify in one pass: keys and signatures in the compressed wire format (what
 * PublicKey.Serialize / Signature.Serialize produce, g2pubs/bls.go:18-20, 67-69): g2pubs pk 96 B + sig 48 B,
 * g1pubs pk 48 B + sig 96 B.  check_subgroup != 0 applies the subgroup test of DeserializePublicKey /
 * DeserializeSignature.  ok[i] = 0 when either element fails to deserialise or is the point at infinity;
 * err_pk / err_sig (n bytes each, may be NULL) receive the error codes of blsmi_g*_decompress_batch. */
int blsmi_g2pubs_verify_serialized_batch(const uint8_t *msgs, const uint64_t *off /* n+1 */, const uint8_t *pks /* n*96 */, const uint8_t *sigs /* n*48 */,
                                         int check_subgroup, uint8_t *ok /* n */, uint8_t *err_pk, uint8_t *err_sig, size_t n);
int blsmi_g1pubs_verify_serialized_batch(const uint8_t *msgs, const uint64_t *off /* n+1 */, const uint8_t *pks /* n*48 */, const uint8_t *sigs /* n*96 */,
                                         int check_subgroup, uint8_t *ok /* n */, uint8_t *err_pk, uint8_t *err_sig, size_t n);

/* ---- wire format (CompressG1/G2, DecompressG1/G2 incl. subgroup check; g1.go:185-249, g2.go:219-295)
 * err[i]: 0 ok, 1 unexpected compression mode, 2 bad infinity encoding, 3 not on curve, 4 not in subgroup  * check_subgroup: 0 = none, 1 = the subgroup test through the curve endomorphisms (the same predicate as the
 * reference's r*P == infinity for every point on the curve, 4x cheaper), 2 = the r*P form itself. */
int blsmi_g1_decompress_batch(const uint8_t *in /* n*48 */, int check_subgroup, uint8_t *out /* n*96 */, uint8_t *out_inf, uint8_t *err, size_t n);
int blsmi_g2_decompress_batch(const uint8_t *in /* n*96 */, int check_subgroup, uint8_t *out /* n*192 */, uint8_t *out_inf, uint8_t *err, size_t n);
int blsmi_g1_compress_batch(const uint8_t *pts, const uint8_t *in_inf, uint8_t *out /* n*48 */, size_t n);
int blsmi_g2_compress_batch(const uint8_t *pts, const uint8_t *in_inf, uint8_t *out /* n*96 */, size_t n);

/* ---- unit-level device ops, exported for the parity tests (tests/test_gpu_field.py).  Operands are
 * arrays of n records of `width` Fq values, each Fq as 6 LE uint64 Montgomery(2^384) limbs. -------- */
enum blsmi_debug_op {
    BLSMI_OP_FQ_MUL = 1, BLSMI_OP_FQ_SQR, BLSMI_OP_FQ_ADD, BLSMI_OP_FQ_SUB, BLSMI_OP_FQ_NEG, BLSMI_OP_FQ_INV, BLSMI_OP_FQ_SQRT,
    BLSMI_OP_FQ_DBL /* DoubleAssign fq.go:140-143 */, BLSMI_OP_FQ_CMP /* Cmp fq.go:134-137: flag = 0/1/2 for a <,=,> b */, BLSMI_OP_FQ_PARITY /* fq.go:269-273: flag */,
    BLSMI_OP_FQ_LAZY /* (1029 ab + 4a)(4b - 1029 ab): sums and small multiples grown to the limb and value bounds of the device's lazy Fq type, value-reduced, multiplied */,
    BLSMI_OP_FQ2_MUL = 16, BLSMI_OP_FQ2_SQR, BLSMI_OP_FQ2_INV, BLSMI_OP_FQ2_MUL_NR, BLSMI_OP_FQ2_SQRT, BLSMI_OP_FQ2_SQRT_ANY /* either root */, BLSMI_OP_FQ2_PARITY /* fq2.go:256-260: flag */,
    BLSMI_OP_FQ6_MUL = 32, BLSMI_OP_FQ6_SQR, BLSMI_OP_FQ6_INV, BLSMI_OP_FQ6_FROB1,
    BLSMI_OP_FQ6_MUL_BY_1 /* fq6.go:40-57, c1 = b[0..1] */, BLSMI_OP_FQ6_MUL_BY_01 /* fq6.go:60-90, (c0, c1) = b[0..3] */,
    BLSMI_OP_FQ12_MUL = 48, BLSMI_OP_FQ12_SQR, BLSMI_OP_FQ12_INV, BLSMI_OP_FQ12_FROB1, BLSMI_OP_FQ12_FROB2, BLSMI_OP_FQ12_FROB3, BLSMI_OP_FQ12_CYCLO_SQR, BLSMI_OP_FQ12_CYCLO_RUN16 /* 16 squarings in compressed form + decompression */,
    BLSMI_OP_FQ12_MUL_BY_014 /* fq12.go:32-47, (c0, c1, c4) = b[0..5] */, BLSMI_OP_FQ12_MUL_BY_LINE_PAIR /* a * (014 element b[0..5]) * (014 element b[6..11]) through the fused two-line product */,
    BLSMI_OP_FQ12_FINAL_EXP = 58 /* with BLSMI_OP_LANE_PAIR (k_fe_pair.hip, the cores of k_final_exp_pair) or BLSMI_OP_LANE_QUAD only: pairing.go:79-129; zero gives zero */,
    BLSMI_OP_G1_DOUBLE = 64, BLSMI_OP_G1_ADD, BLSMI_OP_G2_DOUBLE, BLSMI_OP_G2_ADD,
    BLSMI_OP_SWU_G1 = 68 /* t in word 0 of a 3-Fq record -> (x, y, 0) */, BLSMI_OP_SWU_G2 /* t in words 0-1 of a 6-Fq record -> (x, y, 0) */,
    BLSMI_OP_G1_MUL_U64 = 70 /* blsmi 0.8: the Jacobian G1 point a times the 64-bit scalar in word 0 of b's record, by the plain ladder of the randomised batch verification */,
    /* with BLSMI_OP_LANE_ROW: one step of the homogeneous Miller loop on a 12-Fq record (X, Y, Z of the running point: Fq2 each; xq, yq of Q:
     * Fq2 each; xP, yP: Fq each) -> (X3, Y3, Z3, c0, c1, c4): the new point and the line at P.  _REF: the lane-pair routine the row form restates.
     * DBL_STEP / ADD_STEP also with BLSMI_OP_LANE_PAIR (doubling_step_h / addition_step_h) and BLSMI_OP_LANE_QUAD (doubling_step_q / addition_step_h) */
    BLSMI_OP_ROW_DBL_STEP = 80, BLSMI_OP_ROW_DBL_STEP_REF, BLSMI_OP_ROW_ADD_STEP, BLSMI_OP_ROW_ADD_STEP_REF,
    /* with BLSMI_OP_LANE_ROW only: G2 Jacobian arithmetic of the row layout's HashG2 tail (row_g2.inc) on a 12-Fq record (X1, Y1, Z1, X2, Y2, Z2: Fq2 each)
     * -> (X3, Y3, Z3, 0, 0, 0): g2.go:389-443 of the first point, g2.go:446-529 of both WITHOUT the special cases (infinity or equal x give Z3 = 0),
     * hash.go:368-389 of the first point */
    BLSMI_OP_ROW_G2_DOUBLE = 84, BLSMI_OP_ROW_G2_ADD, BLSMI_OP_ROW_CLEAR_H2
};
#define BLSMI_OP_LANE_PAIR 0x100 /* OR into an FQ2 / FQ6 / FQ12 op or ROW_DBL_STEP / ROW_ADD_STEP: run it in the lane-pair layout of the pairing kernels */
#define BLSMI_OP_LANE_QUAD 0x200 /* OR into an FQ12 op (not MUL_BY_LINE_PAIR) or ROW_DBL_STEP / ROW_ADD_STEP: run it in the lane-quad layout (four lanes per tuple, k_pairing_quad.hip) */
#define BLSMI_OP_LANE_ROW 0x400  /* OR into an FQ12 op (not CYCLO_RUN16, MUL_BY_LINE_PAIR or FINAL_EXP): run it in the lane-row layout (sixteen lanes per tuple, k_pairing_row.hip) */
int blsmi_debug_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint8_t *flag /* n, may be NULL */, size_t n);
/* G2AffineToPrepared (g2.go:650-801) of one affine G2 point: 68 line-coefficient triples, each Fq2 as 12 LE uint64 Montgomery(2^384)
 * limbs, in Miller-loop order.  mode 0: computed by the one-tuple-per-lane doubling/addition steps; 1: by the lane-pair
 * steps; 2: the table of the G2 generator the library prepared at start-up for g2pubs.Verify (g2_aff ignored). */
int blsmi_debug_g2_prepare(const uint8_t *g2_aff /* 192 */, int mode, uint64_t *out /* 68*3*12 */);

/* The two halves of a small-batch hash-to-curve, for the parity tests.  kind 0 / 1 / 2 = HashG1 (hash.go:326-331) / HashG2
 * (hash.go:405-411) / HashG2WithDomain (g2.go:1041-1085).
 * blsmi_debug_hash_tail: the curve arithmetic after the SWU maps (isogeny, sum, cofactor clearing; kind 2: ScaleByCofactor)
 * run as a level program of the latency path.  pts: per message the mapped affine points as big-endian 48-byte field
 * elements -- kind 0: two points of the 11-isogenous curve (192 bytes), kind 1: two points of the 3-isogenous curve (384),
 * kind 2: the point of E'(Fq2) the try-and-increment search found (192).  out: the hash point (96 / 192 / 192 bytes);
 * good[i] = 0 when message i met an exceptional step (the library then re-hashes it with the kernel below).
 * blsmi_debug_hash_redo: that kernel -- messages with good[i] == 0 are hashed by the one-message-per-lane routine into
 * out[i]; the records of the others are left as they were.  n <= 4096 for the tail. */
int blsmi_debug_hash_tail(int kind, const uint8_t *pts, uint8_t *out, uint8_t *good, size_t n);
/* the same tail of HashG1 as the THROUGHPUT kernel runs it (k_hash_g1_finish), with (clear != 0) or without the cofactor clearing of hash.go:306-309;
 * *special gets bit 1 when clear == 0 and some message's two mapped points cancel -- the case a large VerifyAggregate's uncleared-hash path hands
 * back to the cleared one. */
int blsmi_debug_hash_g1_finish(const uint8_t *pts /* n*192 */, int clear /* 2: the four-lanes-per-message tail + its redo pass; *special = messages redone */, uint8_t *out /* n*96 */, int *special, size_t n);
int blsmi_debug_hash_redo(int kind, const uint8_t *msgs, const uint64_t *off_or_domain, const uint8_t *good, uint8_t *out /* in/out */, size_t n);
/* One launch of unit program `which` of the latency path (bls_amd/csrc/gen_lat.py: UNIT_PROGRAMS, in that order): single job kinds at the
 * bounds the program generator admits, for the parity tests.  in_raw: n tuples of nin field elements in the device representation, 15 int32
 * limbs each, taken as they are (|limb| <= 2^27 + 64, |value| <= q), array of structures; one wave per tuple.  out_raw: the program's nout
 * results as the kernel left them, limb j of result e of tuple t at ((e * 15) + j) * n + t; ok: the n verdict bytes of the two verdict
 * programs (which write no out_raw; either pointer may be NULL where the program does not write it).  BLSMI_E_ARG for an unknown `which`,
 * an nin that is not the program's, n == 0 or n > 4096. */
int blsmi_debug_lat_unit(int which, const int32_t *in_raw /* n*nin*15 */, size_t nin, size_t n, int32_t *out_raw /* nout*15*n */, uint8_t *ok /* n */);

/* ---- committees (blsmi 0.9) ----------------------------------------------------------------------------------------------------------
 * Segmented sums: m sums over ragged, index-addressed subsets of one table of npk points.  Segment j is
 * {pts[idx[k]] : seg_off[j] <= k < seg_off[j + 1]} (idx NULL: the positions k themselves); seg_off has m + 1 entries, seg_off[0] = 0,
 * non-decreasing.  out: m affine records (the all-zero record for infinity), out_inf[j] = 1 for infinity (the empty segment included),
 * else 0.  Each record is the bytes blsmi_g?_sum gives for the gathered points, whatever "segsum_chunk" is.  The host forms check
 * the offsets and every index (< npk) and return BLSMI_E_ARG before any device work; the _dev forms read seg_off back to the host
 * (offsets that do not start at 0 or decrease: BLSMI_E_ARG) and mark a segment holding an index >= npk with out_inf = 2 and the
 * all-zero record, reading nothing past the table.  _jac: the points as the Go values hold them (144 / 288 bytes each, z == 0 is
 * infinity, no in_inf).  m = 0 returns BLSMI_OK. */
int blsmi_g1_sum_segmented(const uint8_t *pts /* npk*96 */, const uint8_t *in_inf /* npk, may be NULL */, size_t npk,
                           const uint32_t *idx /* seg_off[m], may be NULL */, const uint64_t *seg_off /* m+1 */, size_t m,
                           uint8_t *out /* m*96 */, uint8_t *out_inf /* m */);
int blsmi_g2_sum_segmented(const uint8_t *pts /* npk*192 */, const uint8_t *in_inf /* npk, may be NULL */, size_t npk,
                           const uint32_t *idx /* seg_off[m], may be NULL */, const uint64_t *seg_off /* m+1 */, size_t m,
                           uint8_t *out /* m*192 */, uint8_t *out_inf /* m */);
int blsmi_g1_sum_segmented_jac(const uint64_t *pts_jac /* npk*18 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off, size_t m,
                               uint8_t *out /* m*96 */, uint8_t *out_inf /* m */);
int blsmi_g2_sum_segmented_jac(const uint64_t *pts_jac /* npk*36 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off, size_t m,
                               uint8_t *out /* m*192 */, uint8_t *out_inf /* m */);
int blsmi_g1_sum_segmented_dev(const void *d_pts, const void *d_in_inf, size_t npk, const void *d_idx, const void *d_seg_off, size_t m,
                               void *d_out, void *d_out_inf, void *stream);
int blsmi_g2_sum_segmented_dev(const void *d_pts, const void *d_in_inf, size_t npk, const void *d_idx, const void *d_seg_off, size_t m,
                               void *d_out, void *d_out_inf, void *stream);
/* Weighted segmented sums (blsmi 0.11), a 64-bit segmented MSM: segment j is sum scalars[idx[k]] * pts[idx[k]] over seg_off[j] <= k <
 * seg_off[j + 1] -- the scalar is addressed by the same index as the point.  Arguments, checks and BLSMI_E_ARG rules as
 * blsmi_g?_sum_segmented, plus scalars (npk words, NULL with npk > 0: BLSMI_E_ARG).  A zero scalar is allowed and contributes nothing, as
 * a point flagged in in_inf does.  Each record is the bytes blsmi_g?_sum gives for the multiples, whatever "segsum_chunk" is. */
int blsmi_g1_sum_segmented_u64(const uint8_t *pts /* npk*96 */, const uint8_t *in_inf /* npk, may be NULL */, size_t npk, const uint64_t *scalars /* npk */,
                               const uint32_t *idx /* seg_off[m], may be NULL */, const uint64_t *seg_off /* m+1 */, size_t m,
                               uint8_t *out /* m*96 */, uint8_t *out_inf /* m */);
int blsmi_g2_sum_segmented_u64(const uint8_t *pts /* npk*192 */, const uint8_t *in_inf /* npk, may be NULL */, size_t npk, const uint64_t *scalars /* npk */,
                               const uint32_t *idx /* seg_off[m], may be NULL */, const uint64_t *seg_off /* m+1 */, size_t m,
                               uint8_t *out /* m*192 */, uint8_t *out_inf /* m */);
/* Batches of VerifyAggregateCommon (g2pubs/bls.go:275-278, g1pubs/bls.go:287-297).  Item j:
 *   VerifyAggregateCommon(sig_j, {pks[idx[k]] : seg_off[j] <= k < seg_off[j + 1]}, msg_j)
 * with msg_j = msgs[msg_off[j] .. msg_off[j + 1]) (with_domain: the 32 bytes msgs32 + 32 j under the common 8-byte domain).  Each verdict
 * is exactly what the single-call entry point returns for that committee, message and signature: 0 for an empty committee, for one that
 * sums to infinity and for the all-zero signature record.  The committee sums run beside the hash of the m messages, then the m checks
 * run as one verify batch of m tuples, on one device.  ok: m verdict bytes, ok_bitmap: (m + 7) / 8 bytes, LSB first; either may be NULL,
 * not both.  The host forms check offsets and indices as the segmented sums do (BLSMI_E_ARG); the _dev forms take every buffer on one of
 * the library's devices (d_ok: m bytes; d_msg_off / d_domain as blsmi_g?pubs_verify_batch_dev) and give verdict 0 to an item whose
 * committee holds an index >= npk.  _jac: keys and signatures as the Go values hold them.  m = 0 returns BLSMI_OK. */
int blsmi_g2pubs_verify_aggregate_common_batch(const uint8_t *msgs, const uint64_t *msg_off /* m+1 */, const uint8_t *pks /* npk*192 */, size_t npk,
                                               const uint32_t *idx, const uint64_t *seg_off /* m+1 */, const uint8_t *sigs /* m*96 */,
                                               uint8_t *ok /* m, may be NULL */, uint8_t *ok_bitmap /* may be NULL */, size_t m);
int blsmi_g1pubs_verify_aggregate_common_batch(const uint8_t *msgs, const uint64_t *msg_off /* m+1 */, const uint8_t *pks /* npk*96 */, size_t npk,
                                               const uint32_t *idx, const uint64_t *seg_off /* m+1 */, const uint8_t *sigs /* m*192 */,
                                               uint8_t *ok, uint8_t *ok_bitmap, size_t m);
int blsmi_g1pubs_verify_aggregate_common_with_domain_batch(const uint8_t *msgs32 /* m*32 */, const uint8_t domain[8], const uint8_t *pks /* npk*96 */, size_t npk,
                                                           const uint32_t *idx, const uint64_t *seg_off /* m+1 */, const uint8_t *sigs /* m*192 */,
                                                           uint8_t *ok, uint8_t *ok_bitmap, size_t m);
int blsmi_g2pubs_verify_aggregate_common_batch_jac(const uint8_t *msgs, const uint64_t *msg_off, const uint64_t *pks /* npk*36 */, size_t npk,
                                                   const uint32_t *idx, const uint64_t *seg_off, const uint64_t *sigs /* m*18 */,
                                                   uint8_t *ok, uint8_t *ok_bitmap, size_t m);
int blsmi_g1pubs_verify_aggregate_common_batch_jac(const uint8_t *msgs, const uint64_t *msg_off, const uint64_t *pks /* npk*18 */, size_t npk,
                                                   const uint32_t *idx, const uint64_t *seg_off, const uint64_t *sigs /* m*36 */,
                                                   uint8_t *ok, uint8_t *ok_bitmap, size_t m);
int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_jac(const uint8_t *msgs32, const uint8_t domain[8], const uint64_t *pks /* npk*18 */, size_t npk,
                                                               const uint32_t *idx, const uint64_t *seg_off, const uint64_t *sigs /* m*36 */,
                                                               uint8_t *ok, uint8_t *ok_bitmap, size_t m);
int blsmi_g2pubs_verify_aggregate_common_batch_dev(const void *d_msgs, const void *d_msg_off, const void *d_pks, size_t npk, const void *d_idx,
                                                   const void *d_seg_off, const void *d_sigs, void *d_ok, size_t m, void *stream);
int blsmi_g1pubs_verify_aggregate_common_batch_dev(const void *d_msgs, const void *d_msg_off, const void *d_pks, size_t npk, const void *d_idx,
                                                   const void *d_seg_off, const void *d_sigs, void *d_ok, size_t m, void *stream);
int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_dev(const void *d_msgs32, const void *d_domain, const void *d_pks, size_t npk, const void *d_idx,
                                                               const void *d_seg_off, const void *d_sigs, void *d_ok, size_t m, void *stream);

/* ---- pairing products (blsmi 0.10) -------------------------------------------------------------------------------------------------
 * m products of pairings, each final-exponentiated once -- the reference's central primitive, bls.MillerLoop(items []MillerLoopItem)
 * followed by bls.FinalExponentiation (pairing.go:16-75, 79-129), m times in one call:
 *   item j = FinalExponentiation(MillerLoop({(P_k, Q_k) : seg_off[j] <= k < seg_off[j + 1]}))
 * Output: out_fq12[j] (72 u64) is in the output format of blsmi_pairing_batch; is_one[j] = 1 exactly when that value equals FQ12One -- for
 * a two-pair segment with a negated P this is CompareTwoPairings (pairing.go:140-147).  Either output may be NULL, not both (BLSMI_E_ARG).
 * Infinity: a pair whose P or Q is at infinity contributes 1 (what the reference intends; the Go code itself would panic).  Infinity is
 * a flag (inf_flags[k] bit 0: P_k, bit 1: Q_k; the array may be NULL), the all-zero record, or z == 0 in the _jac forms (144 / 288 bytes
 * a point, as the Go values hold them).  An empty segment, or one whose pairs are all skipped, gives FQ12One and is_one = 1.
 * Offsets: m + 1 entries, seg_off[0] = 0, non-decreasing, seg_off[m] = np.  The host forms check this, and NULL inputs with np > 0, and
 * return BLSMI_E_ARG before any device work; the _dev forms read the offsets back to the host as the segmented sums do and return the
 * same error.  m = 0 returns BLSMI_OK; np = 0 with m > 0 is legal: every item is one.
 * A single-pair segment gives exactly the bytes of blsmi_pairing_batch for that pair, and every result is bit-identical whatever layouts
 * the stages take: one Miller value per pair in the layout a Pairing call of np tuples takes, the segmented Fq12 product a row of sixteen
 * lanes per chunk of K consecutive values (K: the "segsum_chunk" option, chosen from np as the segmented sums choose it from their total),
 * the final exponentiation of the m products in the layout blsmi_final_exponentiation_batch gives m values (more than the latency
 * threshold: a Pairing call's four- / two-lane kernels).  The call runs on ONE device: it is not sharded and does not join the request
 * combiner.  The _dev forms take every buffer on one of the library's devices (d_out_fq12: m*576 bytes, d_is_one: m bytes, d_seg_off:
 * (m + 1) u64) and leave the caller's point buffers untouched. */
int blsmi_pairing_product_batch(const uint8_t *g1_aff /* np*96 */, const uint8_t *g2_aff /* np*192 */,
                                const uint8_t *inf_flags /* np, may be NULL: bit0 = P_k infinity, bit1 = Q_k infinity */, size_t np,
                                const uint64_t *seg_off /* m+1 */, size_t m,
                                uint64_t *out_fq12 /* m*72, may be NULL */, uint8_t *is_one /* m, may be NULL */);
int blsmi_pairing_product_batch_jac(const uint64_t *g1_jac /* np*18 */, const uint64_t *g2_jac /* np*36 */, size_t np,
                                    const uint64_t *seg_off, size_t m, uint64_t *out_fq12, uint8_t *is_one);
int blsmi_pairing_product_batch_dev(const void *d_g1_aff, const void *d_g2_aff, const void *d_inf_flags, size_t np,
                                    const void *d_seg_off, size_t m, void *d_out_fq12, void *d_is_one, void *stream);
int blsmi_pairing_product_batch_jac_dev(const void *d_g1_jac, const void *d_g2_jac, size_t np,
                                        const void *d_seg_off, size_t m, void *d_out_fq12, void *d_is_one, void *stream);

/* ---- point validation (blsmi 0.14) ---------------------------------------------------------------------------------------------------
 * The tool behind every "PRECONDITION: ... in the prime-order subgroups" above: G?Affine.IsOnCurve (g1.go:93-105, g2.go:118-130) and
 * IsInCorrectSubgroupAssumingOnCurve (g1.go:137-141, g2.go:293-295) of n points in the form the caller holds them, without the detour
 * through compress + decompress(check).  status[i] is one of the BLSMI_POINT_* values below; NOT_ON_CURVE and NOT_IN_SUBGROUP are
 * deliberately the error codes 3 and 4 of blsmi_g?_decompress_batch.  A point is usable where the reference's
 * IsOnCurve() && IsInCorrectSubgroupAssumingOnCurve() holds: status OK or INFINITY (the reference returns true for infinity in both).
 *   check   as in the decompression calls: 0 the curve equation only (NOT_IN_SUBGROUP never appears), 1 the subgroup test through the
 *           curve's endomorphisms ([x^2] P + phi(P) on G1, [|x|] P + psi(P) on G2), 2 the reference's r * P == infinity walk (same
 *           verdicts, ~4x / ~2x the work).  Any other value: BLSMI_E_ARG.
 *   order   infinity gives INFINITY; otherwise a failed curve equation gives NOT_ON_CURVE and the subgroup test, which assumes a curve
 *           point, is not consulted; otherwise a failed subgroup test gives NOT_IN_SUBGROUP.
 *   records are read exactly as every other entry point reads them.  Infinity is the all-zero affine record, a set in_inf byte, or
 *           z == 0 in a Jacobian record (whatever x and y hold).  A coordinate whose big-endian value (affine) or limb image (Jacobian)
 *           is not below q is read as 0, as everywhere in this library, and the point is judged AS THAT POINT: an affine record with
 *           x >= q is the point (0, y).
 *   cost    the curve equation is tested on the coordinates as they arrive (Jacobian: Y^2 == X^3 + b Z^6) and the subgroup verdict is
 *           the infinity flag of a sum: no field inversion and no square root, one kernel launch for every n.
 * n == 0 returns BLSMI_OK; NULL pts or status with n > 0 is BLSMI_E_ARG before any device work.  The call runs on ONE device: it is not
 * sharded and does not join the request combiner.  The _dev forms take every buffer on one of the library's devices (d_status: n bytes;
 * jac != 0: d_pts holds Jacobian records and d_in_inf must be NULL, else BLSMI_E_ARG) and leave the caller's point buffers untouched.
 * G2 runs a lane pair per point by default and one lane per point under BLSMI_LAYOUT=single; the statuses are the same. */
#define BLSMI_POINT_OK 0              /* a finite point of the prime-order subgroup (check 0: of the curve) */
#define BLSMI_POINT_INFINITY 1        /* the point at infinity */
#define BLSMI_POINT_NOT_ON_CURVE 3    /* = the decompression error "x is not on the curve" */
#define BLSMI_POINT_NOT_IN_SUBGROUP 4 /* on the curve, outside the prime-order subgroup (= the decompression error 4) */
int blsmi_g1_check_batch(const uint8_t *pts /* n*96 */, const uint8_t *in_inf /* n, may be NULL */, int check, uint8_t *status /* n */, size_t n);
int blsmi_g2_check_batch(const uint8_t *pts /* n*192 */, const uint8_t *in_inf /* n, may be NULL */, int check, uint8_t *status /* n */, size_t n);
int blsmi_g1_check_batch_jac(const uint64_t *pts_jac /* n*18 */, int check, uint8_t *status /* n */, size_t n);
int blsmi_g2_check_batch_jac(const uint64_t *pts_jac /* n*36 */, int check, uint8_t *status /* n */, size_t n);
int blsmi_g1_check_batch_dev(const void *d_pts, const void *d_in_inf, int jac, int check, void *d_status, size_t n, void *stream);
int blsmi_g2_check_batch_dev(const void *d_pts, const void *d_in_inf, int jac, int check, void *d_status, size_t n, void *stream);

/* ---- the wire format <-> in-memory points (blsmi 0.15) ---------------------------------------------------------------------------------
 * Deserialize and Serialize for the points as the Go values hold them (144 / 288 bytes, "in-memory points at the boundary" above), n at a
 * time: what arrives compressed can go straight into any *_jac entry point, and what a *_jac entry point returned can leave compressed,
 * without affine records visiting the host.  Each call is defined by the entry points that already exist:
 *   decompress_batch_jac   DecompressG?(b).ToProjective().  err[i] and out_inf[i] (may be NULL) are exactly what blsmi_g?_decompress_batch
 *           gives for the same bytes and the same check_subgroup (0 / 1 / 2; any other value: BLSMI_E_ARG).  out_jac[i] is the in-memory
 *           form of that call's record: (x, y, 1) in Montgomery limbs for a usable finite point, and (0, 1, 0) -- the reference's
 *           G?ProjectiveZero -- for a well-formed infinity encoding AND for every record with err != 0, so that a downstream *_jac call
 *           gives a tuple with an undecodable element verdict 0 (z == 0) without reading err.
 *   compress_batch_jac     CompressG?(p.ToAffine()).  out[i] is the bytes blsmi_g?_compress_batch gives for the record and flag that
 *           blsmi_g?_jac_to_affine_batch gives for pts_jac[i]: z == 0 gives 0xc0 followed by zeros whatever x and y hold, a limb image not
 *           below q reads as 0, and there is no curve test.  One kernel launch for every n, one lane per point; a wave whose points all
 *           have z == 1 skips the inversion.
 * n == 0 returns BLSMI_OK; a NULL required buffer with n > 0 is BLSMI_E_ARG before any device work.  The host forms run on ONE device: they
 * are not sharded and do not join the request combiner.  The _dev forms take every buffer on one of the library's devices (stream as in
 * blsmi_pairing_batch_dev); input and output must not overlap, and the caller's input is left untouched. */
int blsmi_g1_decompress_batch_jac(const uint8_t *in /* n*48 */, int check_subgroup, uint64_t *out_jac /* n*18 */, uint8_t *out_inf /* n, may be NULL */,
                                  uint8_t *err /* n */, size_t n);
int blsmi_g2_decompress_batch_jac(const uint8_t *in /* n*96 */, int check_subgroup, uint64_t *out_jac /* n*36 */, uint8_t *out_inf /* n, may be NULL */,
                                  uint8_t *err /* n */, size_t n);
int blsmi_g1_compress_batch_jac(const uint64_t *pts_jac /* n*18 */, uint8_t *out /* n*48 */, size_t n);
int blsmi_g2_compress_batch_jac(const uint64_t *pts_jac /* n*36 */, uint8_t *out /* n*96 */, size_t n);
int blsmi_g1_decompress_batch_jac_dev(const void *d_in, int check_subgroup, void *d_out_jac, void *d_out_inf /* may be NULL */, void *d_err, size_t n, void *stream);
int blsmi_g2_decompress_batch_jac_dev(const void *d_in, int check_subgroup, void *d_out_jac, void *d_out_inf /* may be NULL */, void *d_err, size_t n, void *stream);
int blsmi_g1_compress_batch_jac_dev(const void *d_pts_jac, void *d_out, size_t n, void *stream);
int blsmi_g2_compress_batch_jac_dev(const void *d_pts_jac, void *d_out, size_t n, void *stream);

/* ---- committee aggregates, randomised (blsmi 0.16) -----------------------------------------------------------------------------------
 * "Verify multiple aggregate signatures": the batches of VerifyAggregateCommon of "committees" above under the ONE equation of the grouped
 * randomised form.  A block's attestations, a slot's gossip aggregates: m signature sets (signature, committee of the registry, message),
 * usually with far fewer distinct messages than sets.  Item j is
 *   VerifyAggregateCommon(sig_j, {pks[idx[k]] : seg_off[j] <= k < seg_off[j + 1]}, table[msg_idx[j]])
 * The message table and msg_idx are those of *_verify_batch_rlc_grouped: msgs with msg_off[d + 1] (with_domain: msgs32, d * 32 bytes, and
 * the 8-byte domain), then msg_idx[m].  The registry pks[npk], idx (NULL: the positions k themselves) and seg_off[m + 1] are those of
 * *_verify_aggregate_common_batch.  sigs: m records.  scalars: m nonzero 64-bit words, or NULL to have them drawn from the OS for this
 * call.  ok: m verdict bytes, ok_bitmap: (m + 7) / 8 bytes, LSB first; either may be NULL, not both.  With apk_j the sum of committee j:
 *     g1pubs: e(G1gen, sum_j r_j sig_j) == prod_g e(sum_{j in g} r_j apk_j, H(m_g))
 *     g2pubs: e(sum_j r_j sig_j, G2gen) == prod_g e(H(m_g), sum_{j in g} r_j apk_j)
 * one hash and one Miller loop per table entry some item refers to and ONE final exponentiation, where the 0.9 call runs m hashes, 2m
 * Miller loops and m final exponentiations.  The committee sums run beside the hash as they do there; both weighted sums run a 64-bit
 * ladder per item (G2: a lane pair per item by default, one lane under BLSMI_LAYOUT=single; the same points either way).
 * Verdicts: ok[j] is exactly what *_verify_aggregate_common*_batch gives for the same inputs -- 0 for an empty committee, for one that
 * sums to infinity, for the all-zero signature record and (the _dev forms) for a committee holding an index >= npk.  *combined (may be
 * NULL) = 1 exactly when every verdict came from the one equation that held; otherwise the equation failed or a flagged item met it, and
 * the m Verify()s of the 0.9 call ran from what was on the device (the check is not narrowed to blocks or cells here).
 * Soundness: with an invalid item among them the equation holds with probability at most 2^-64 over the drawn scalars, keys and
 * signatures in the prime-order subgroups (as Deserialize guarantees).  The weights are per ITEM also inside a message's group: with caller
 * scalars r_a == r_b two items of one message may swap signatures unnoticed -- the caller's responsibility, as every caller scalar is.
 *   - the host forms return BLSMI_E_ARG before any device work for: offsets that do not start at 0 or decrease, an index >= npk,
 *     msg_idx[j] >= d (d = 0 with m > 0 included), a zero caller scalar, a NULL input with m > 0, both outputs NULL.
 *     m = 0: BLSMI_OK, combined = 0.
 *   - table entries with equal bytes are not merged; the host forms never hash an entry no item refers to.
 *   - _jac: registry and signatures as the Go values hold them (G?Projective records, z == 0 is infinity), no infinity flags.
 *   - _dev: every buffer on one of the library's devices, as the 0.9 _dev forms take them (affine records; d_msg_off / d_domain; d_ok: m
 *     bytes), plus d_msg_idx (m u32).  scalars and combined stay on the host.  seg_off and msg_idx are read back once for the plans
 *     (offsets that do not start at 0 or decrease, msg_idx[j] >= d: BLSMI_E_ARG); every table entry is hashed.
 * "rlc_min" does NOT apply: calling this form is the caller's choice of the combined path, at any m.  The call takes one lease and runs on
 * one device; it is not split and never joins the request combiner.  DESIGN.md 3q has the shapes at which it wins and loses against the
 * 0.9 call. */
int blsmi_g2pubs_verify_aggregate_common_batch_rlc(const uint8_t *msgs, const uint64_t *msg_off /* d+1 */, size_t d, const uint32_t *msg_idx /* m */,
                                                   const uint8_t *pks /* npk*192 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off /* m+1 */,
                                                   const uint8_t *sigs /* m*96 */, const uint64_t *scalars /* m, may be NULL */,
                                                   uint8_t *ok /* m, may be NULL */, uint8_t *ok_bitmap /* may be NULL */, size_t m, int *combined);
int blsmi_g1pubs_verify_aggregate_common_batch_rlc(const uint8_t *msgs, const uint64_t *msg_off /* d+1 */, size_t d, const uint32_t *msg_idx /* m */,
                                                   const uint8_t *pks /* npk*96 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off /* m+1 */,
                                                   const uint8_t *sigs /* m*192 */, const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t m, int *combined);
int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc(const uint8_t *msgs32 /* d*32 */, const uint8_t domain[8], size_t d, const uint32_t *msg_idx /* m */,
                                                               const uint8_t *pks /* npk*96 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off /* m+1 */,
                                                               const uint8_t *sigs /* m*192 */, const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t m, int *combined);
int blsmi_g2pubs_verify_aggregate_common_batch_rlc_jac(const uint8_t *msgs, const uint64_t *msg_off, size_t d, const uint32_t *msg_idx,
                                                       const uint64_t *pks /* npk*36 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off,
                                                       const uint64_t *sigs /* m*18 */, const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t m, int *combined);
int blsmi_g1pubs_verify_aggregate_common_batch_rlc_jac(const uint8_t *msgs, const uint64_t *msg_off, size_t d, const uint32_t *msg_idx,
                                                       const uint64_t *pks /* npk*18 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off,
                                                       const uint64_t *sigs /* m*36 */, const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t m, int *combined);
int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac(const uint8_t *msgs32, const uint8_t domain[8], size_t d, const uint32_t *msg_idx,
                                                                   const uint64_t *pks /* npk*18 */, size_t npk, const uint32_t *idx, const uint64_t *seg_off,
                                                                   const uint64_t *sigs /* m*36 */, const uint64_t *scalars, uint8_t *ok, uint8_t *ok_bitmap, size_t m, int *combined);
int blsmi_g2pubs_verify_aggregate_common_batch_rlc_dev(const void *d_msgs, const void *d_msg_off, size_t d, const void *d_msg_idx, const void *d_pks, size_t npk,
                                                       const void *d_idx, const void *d_seg_off, const void *d_sigs, const uint64_t *scalars /* host: m, may be NULL */,
                                                       void *d_ok, size_t m, int *combined /* host */, void *stream);
int blsmi_g1pubs_verify_aggregate_common_batch_rlc_dev(const void *d_msgs, const void *d_msg_off, size_t d, const void *d_msg_idx, const void *d_pks, size_t npk,
                                                       const void *d_idx, const void *d_seg_off, const void *d_sigs, const uint64_t *scalars, void *d_ok, size_t m,
                                                       int *combined, void *stream);
int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_dev(const void *d_msgs32, const void *d_domain, size_t d, const void *d_msg_idx, const void *d_pks, size_t npk,
                                                                   const void *d_idx, const void *d_seg_off, const void *d_sigs, const uint64_t *scalars, void *d_ok, size_t m,
                                                                   int *combined, void *stream);
/* For the parity tests: blsmi_g2_sum_segmented_u64 (arguments, checks and bytes) with pass 1 through the lane-pair ladder
 * k_g2_segsum_chunk_u64_pair whatever BLSMI_LAYOUT says -- the kernel the call above takes by default. */
int blsmi_debug_g2_sum_segmented_u64_pair(const uint8_t *pts /* npk*192 */, const uint8_t *in_inf /* npk, may be NULL */, size_t npk, const uint64_t *scalars /* npk */,
                                          const uint32_t *idx /* seg_off[m], may be NULL */, const uint64_t *seg_off /* m+1 */, size_t m,
                                          uint8_t *out /* m*192 */, uint8_t *out_inf /* m */);

/* ---- pairing products, randomised (blsmi 0.17) -----------------------------------------------------------------------------------------
 * The m equations "item j is one" of blsmi_pairing_product_batch (Groth16 proofs, KZG openings, two-sided checks) under ONE randomised
 * equation, for batches whose G2 points are mostly fixed.  Pair k is (P_k, g2_tab[q_idx[k]]): the G2 points come from a table of nq entries
 * (q_idx NULL: pair k uses entry k, and nq must equal np); item j is the pairs seg_off[j] <= k < seg_off[j + 1], as in 0.10.  With random
 * nonzero 64-bit r_j per item, item(k) the item of pair k and FE the final exponentiation,
 *     every item j holds  <=  FE( prod_g Miller( sum_{k: q_idx[k] = g} r_item(k) * P_k , Q_g ) ) == FQ12One
 * by bilinearity: ONE Miller loop per table entry some pair refers to, ONE final exponentiation and a 64-bit G1 ladder per pair, where the
 * 0.10 call runs np Miller loops and m final exponentiations.
 * Verdicts: is_one[j] is exactly what blsmi_pairing_product_batch gives item j with Q_k = g2_tab[q_idx[k]].  There is no out_fq12: the
 * combined path never has per-item values.  *combined (may be NULL) = 1 exactly when every verdict came from the one equation that held;
 * otherwise the equation failed and the 0.10 path ran over all m items from what is on the device (the table entries gathered per pair;
 * the check is not narrowed to blocks here).
 * Infinity follows 0.10: the pair contributes 1.  An infinite P_k (inf_flags[k] bit 0, the all-zero record, z == 0 in the _jac forms) adds
 * nothing to its entry's sum; an infinite table entry (the all-zero record, z == 0) drops its group; a group whose weighted sum is the
 * point at infinity contributes 1 and does NOT send the call to the per-item path -- unlike the signature forms, where a sum at infinity
 * is suspicious: an item {(P, Q), (-P, Q)} is a legitimate equation.
 * Scalars: m nonzero 64-bit words, or NULL to have them drawn from the OS for this call (as 0.8 and 0.16); a zero caller scalar is
 * BLSMI_E_ARG; caller scalars are the caller's responsibility (two failing items whose values cancel under equal scalars pass unnoticed).
 * Soundness: with an item that does not hold among them the equation holds with probability at most 2^-64 over the drawn scalars, for P_k
 * in G1 and table entries in G2, both the prime-order subgroups (blsmi_g?_check_batch establishes that; a point outside them voids it).
 *   - the host forms return BLSMI_E_ARG before any device work for: offsets that do not start at 0, that decrease or that do not end at
 *     np; q_idx[k] >= nq; q_idx == NULL with nq != np; a zero scalar; a NULL input with np > 0; NULL is_one.
 *   - m = 0: BLSMI_OK, combined = 0.  np = 0 with m > 0: every item is one, combined = 1.
 *   - table entries with equal bytes are not merged; entries no pair refers to are never touched (the host forms do not upload them, the
 *     _dev forms do not read them).
 *   - _jac: points as the Go values hold them (g1_jac np*18 u64, g2_tab_jac nq*36 u64), no flags: z == 0 is infinity.
 *   - _dev: every buffer on one of the library's devices (d_q_idx: np u32 or NULL, d_seg_off: (m + 1) u64, d_is_one: m bytes); scalars and
 *     combined stay on the host; `stream` as in blsmi_pairing_batch_dev.  seg_off and q_idx are read back once for the plans (the same
 *     errors, BLSMI_E_ARG, nothing written); the caller's buffers stay untouched.
 * "rlc_min" does NOT apply: calling this form is the caller's choice of the combined path.  The call takes one lease and runs on one
 * device; it is not split and never joins the request combiner.
 * When to call it (one MI355X, points resident, against blsmi_pairing_product_batch_dev on the same pairs, median of 20; DESIGN.md 3r has
 * the table and the stages).  All items valid, m x k pairs: 16 384 x 4 with three shared entries 10.2 against 12.6 ms, 65 536 x 4 the same
 * way 24.3 against 42.1 ms, 16 384 x 2 with both entries shared 4.3 against 8.7 ms.  Do NOT call it with nothing shared (16 384 x 4 under
 * q_idx == NULL: 11.8 against 12.1 ms, a tie within the spread), at a few thousand items or fewer (2 048 x 4: 5.4 against 3.3 ms -- the
 * ladders and the one-value final exponentiation are a floor of about 4 ms), or where failing items are common: one bad item costs this
 * call plus the whole 0.10 call (16 384 x 4: 22.7 against 12.1 ms). */
int blsmi_pairing_product_batch_rlc(const uint8_t *g1_aff /* np*96 */, const uint8_t *inf_flags /* np, may be NULL: bit0 = P_k infinity */,
                                    const uint8_t *g2_tab /* nq*192 */, size_t nq, const uint32_t *q_idx /* np, or NULL: pair k uses entry k and nq == np */,
                                    size_t np, const uint64_t *seg_off /* m+1 */, size_t m,
                                    const uint64_t *scalars /* m, may be NULL */, uint8_t *is_one /* m */, int *combined /* may be NULL */);
int blsmi_pairing_product_batch_rlc_jac(const uint64_t *g1_jac /* np*18 */, const uint64_t *g2_tab_jac /* nq*36 */, size_t nq, const uint32_t *q_idx,
                                        size_t np, const uint64_t *seg_off, size_t m, const uint64_t *scalars, uint8_t *is_one, int *combined);
int blsmi_pairing_product_batch_rlc_dev(const void *d_g1_aff, const void *d_inf_flags, const void *d_g2_tab, size_t nq, const void *d_q_idx,
                                        size_t np, const void *d_seg_off, size_t m, const uint64_t *scalars /* host: m, may be NULL */,
                                        void *d_is_one, int *combined /* host */, void *stream);
int blsmi_pairing_product_batch_rlc_jac_dev(const void *d_g1_jac, const void *d_g2_tab_jac, size_t nq, const void *d_q_idx,
                                            size_t np, const void *d_seg_off, size_t m, const uint64_t *scalars, void *d_is_one, int *combined, void *stream);
/* For the measurement of DESIGN.md 3r: blsmi_pairing_product_batch_rlc_dev (arguments, checks and verdicts) with the single-pair groups
 * sent through the weighted segmented sum like the shared ones, instead of one lane each. */
int blsmi_debug_pairing_product_batch_rlc_dev_nosplit(const void *d_g1_aff, const void *d_inf_flags, const void *d_g2_tab, size_t nq, const void *d_q_idx,
                                                      size_t np, const void *d_seg_off, size_t m, const uint64_t *scalars, void *d_is_one, int *combined,
                                                      void *stream);

/* ---- pairing products, randomised, that find the bad items by blocks (blsmi 0.18) -------------------------------------------------------
 * blsmi_pairing_product_batch_rlc* above, for batches in which an item may fail: arguments, verdicts, infinity rules, scalars and the
 * subgroup precondition are those of 0.17, and two arguments are added -- `block` after `scalars`, `rechecked` (host, may be NULL) after
 * `combined`.  The m items are cut into B = ceil(m / block) contiguous blocks, the last one possibly shorter; block = 0 is automatic,
 * max(64, ceil(m / 256)); any value >= 1 is legal (every cell below has a Miller loop of its own, no layout pairs two of them), and
 * block >= m gives one block.  A CELL is (block b, table entry g) with at least one pair of block b referring to g; with
 *     S_c = sum_{k in c} r_item(k) * P_k,        V_b = prod_{c in b} Miller(S_c, Q_g(c)),        total = prod_b V_b
 * *combined (may be NULL) = 1 exactly when FE(total) == FQ12One: every verdict is 1 then and *rechecked = 0.  When the total fails, the B
 * block values -- which exist by then: no second ladder, no second Miller loop -- are final-exponentiated; the items of the blocks whose
 * value is one get verdict 1, and the items of the failing blocks, and only those, get the verdicts of blsmi_pairing_product_batch's own
 * path.  *rechecked is the number of those items.
 * Soundness: a block whose equation holds has a failing item with probability at most 2^-64 over the drawn scalars, because its weights
 * are its own items'; caller scalars keep 0.17's caveat -- two failing items whose values cancel under equal scalars pass unnoticed, in one
 * block or in two, because the total holds.  P_k and the table entries are in the prime-order subgroups, as in 0.17.
 * Infinity, per cell: an infinite P_k adds nothing to its cell; an all-zero entry drops its cells; a cell whose sum is the point at
 * infinity contributes 1; none of these sends anything to the per-item path; a block with no surviving cell, or with no pairs at all, has
 * value one.
 *   - BLSMI_E_ARG and m = 0 / np = 0 as in 0.17, answered on the host before any device work, with *rechecked = 0.  No `block` value is
 *     refused.  m beyond 2^32 - 1 is BLSMI_E_ARG here (the items of the failing blocks are 32-bit indices).
 *   - _dev: as in 0.17; the caller's buffers stay untouched (the recheck gathers the failing blocks' records into copies of its own).
 * "rlc_min" does NOT apply.  The call takes one lease and runs on one device; it is not split and never joins the request combiner.
 * When to call it (one MI355X, points resident, block = 0, the three calls alternating, median of 20 +- spread in ms; DESIGN.md 3s has the
 * table and the stages): wherever blsmi_pairing_product_batch_rlc_dev is the right call and an item may fail.  One bad item, m x k pairs:
 * 16 384 x 4 with three shared entries 12.5 +- 0.2 against 22.5 +- 0.3 for the 0.17 call (the 0.10 call alone: 11.9), 65 536 x 4 the same
 * way 27.4 +- 0.8 against 66.7 +- 1.0 (0.10: 40.0), 16 384 x 2 with both entries shared 6.6 against 13.2 (0.10: 8.4); sixteen bad items in
 * sixteen blocks cost 0.4 to 2.4 ms more.  All items valid it costs what the 0.17 call costs, within the spreads at the Groth16 shapes
 * (10.2 against 10.2, 24.4 against 24.9) and 0.2 ms LESS at 16 384 x 2 (4.1 against 4.3: the sums' fold passes over 512 cells of 64 pairs are 0.4 ms
 * shorter than over two groups of 16 384, and 512 Miller loops cost what two do, one latency-path launch of 0.7 ms).  What 0.17 says about batches with nothing shared and about a few
 * thousand items or fewer holds here too (2 048 x 4 with one bad item: 7.7 against 3.3 ms for the 0.10 call), and at 16 384 x 4 a failing
 * call is still 0.6 ms behind the 0.10 call alone.  The automatic block stays: at 65 536 x 4 with one bad item, block 64 / 256 / 1 024 /
 * 4 096 give 29.2 / 28.2 / 28.9 / 31.1 ms, spreads 0.7 to 1.0. */
int blsmi_pairing_product_batch_rlc_locate(const uint8_t *g1_aff /* np*96 */, const uint8_t *inf_flags /* np, may be NULL: bit0 = P_k infinity */,
                                           const uint8_t *g2_tab /* nq*192 */, size_t nq, const uint32_t *q_idx /* np, or NULL: pair k uses entry k and nq == np */,
                                           size_t np, const uint64_t *seg_off /* m+1 */, size_t m,
                                           const uint64_t *scalars /* m, may be NULL */, size_t block /* 0 = automatic */,
                                           uint8_t *is_one /* m */, int *combined /* may be NULL */, size_t *rechecked /* may be NULL */);
int blsmi_pairing_product_batch_rlc_locate_jac(const uint64_t *g1_jac /* np*18 */, const uint64_t *g2_tab_jac /* nq*36 */, size_t nq, const uint32_t *q_idx,
                                               size_t np, const uint64_t *seg_off, size_t m, const uint64_t *scalars, size_t block,
                                               uint8_t *is_one, int *combined, size_t *rechecked);
int blsmi_pairing_product_batch_rlc_locate_dev(const void *d_g1_aff, const void *d_inf_flags, const void *d_g2_tab, size_t nq, const void *d_q_idx,
                                               size_t np, const void *d_seg_off, size_t m, const uint64_t *scalars /* host: m, may be NULL */, size_t block,
                                               void *d_is_one, int *combined /* host */, size_t *rechecked /* host */, void *stream);
int blsmi_pairing_product_batch_rlc_locate_jac_dev(const void *d_g1_jac, const void *d_g2_tab_jac, size_t nq, const void *d_q_idx,
                                                   size_t np, const void *d_seg_off, size_t m, const uint64_t *scalars, size_t block,
                                                   void *d_is_one, int *combined, size_t *rechecked, void *stream);

/* ---- scalar-field folds and Groth16 batches (blsmi 0.19) ---------------------------------------------------------------------------------
 * Arithmetic mod r on the device, r the order of G1, G2 and GT:
 *     out[s][0] = sum_{j in segment s} w_j;        out[s][1 + i] = sum_{j in segment s} w_j * vals[j][i] mod r        (i < ncol)
 * vals: n * ncol scalars, row-major, 32-byte big-endian (the library's scalar format); ANY 256-bit value is taken mod r.  weights: n 64-bit
 * words; a zero weight is allowed.  seg_off: nseg + 1 offsets from 0, non-decreasing, n = seg_off[nseg]; an empty segment gives zeros.
 * out: nseg * (ncol + 1) scalars, 32-byte big-endian, every one fully reduced (< r).  One pass over vals: every lane adds unreduced
 * 64 x 256-bit products into twelve 32-bit words, the lanes of a (segment, column) meet with the carries resolved, and there is one
 * reduction mod r per output, not one per row; the result does not depend on how the rows were cut into workgroups.
 *   - BLSMI_E_ARG before any device work: NULL seg_off or out; offsets that do not start at 0 or that decrease; n or ncol beyond
 *     2^32 - 1 (the accumulator's bound); NULL weights with n > 0; NULL vals with n * ncol > 0.  nseg = 0: BLSMI_OK, nothing written.
 *   - _dev: every buffer on one of the library's devices (d_vals 4-byte aligned; read in 16-byte pieces where its address allows);
 *     seg_off is read back once (the same errors); `stream` as in blsmi_pairing_batch_dev; the caller's inputs stay untouched. */
int blsmi_fr_wsum_segmented_u64(const uint8_t *vals /* n*ncol*32 */, size_t ncol, const uint64_t *weights /* n */, const uint64_t *seg_off /* nseg+1 */,
                                size_t nseg, uint8_t *out /* nseg*(ncol+1)*32 */);
int blsmi_fr_wsum_segmented_u64_dev(const void *d_vals, size_t ncol, const void *d_weights, const void *d_seg_off, size_t nseg, void *d_out, void *stream);
/* m Groth16 proofs of one circuit with nin public inputs, from the verifying key, the proofs and the inputs themselves: no L_j is asked of
 * the caller.  vk_g1: alpha, IC_0 .. IC_nin ((nin + 2) records); vk_g2: beta, gamma, delta (3 records); proof_g1: A_j, C_j (2 m records:
 * A_0, C_0, A_1, C_1, ...); proof_g2: B_j (m records); inputs: m * nin scalars, 32-byte big-endian, item-major, taken mod r (NULL allowed
 * when nin == 0).  scalars / block / ok / combined / rechecked exactly as blsmi_pairing_product_batch_rlc_locate.
 * Verdicts: ok[j] is exactly is_one[j] of blsmi_pairing_product_batch on the four pairs (A_j, B_j), (-alpha, beta), (-L_j, gamma),
 * (-C_j, delta), with L_j = IC_0 + sum_i (a_ji mod r) * IC_i computed as blsmi_g1_msm computes it.  Infinity (the all-zero affine record,
 * z == 0 in an in-memory record) follows blsmi_pairing_product_batch: the pair contributes 1; an all-zero vk_g2 entry drops its pairs.
 * The path that holds: per block b of the 0.18 rule (block = 0: max(64, ceil(m / 256))), with the weights r_j,
 *     sum_{j in b} r_j * L_j = t_b * IC_0 + sum_i s_bi * IC_i,        t_b = sum_{j in b} r_j,        s_bi = sum_{j in b} r_j * a_ji mod r
 * -- the fold above over the inputs, the blocks as its segments -- so a block costs nin + 2 full-width ladders (t_b * alpha among them)
 * whatever its length, r_j * A_j goes against its private B_j, sum r_j * C_j against delta, and the blocks' products, the total and one
 * final exponentiation are those of 0.18.  On this path no L_j exists and no item pays a full-width ladder.  When the total fails the
 * block values are final-exponentiated, and for the items of the failing blocks, and only those, L_j is built (nin + 1 ladders each and a
 * segmented sum) and the four pairs go through blsmi_pairing_product_batch's own path; *rechecked is the number of those items.
 * Soundness: the fold is the same group element as sum r_j * L_j only for IC_i of order r, so 0.17's precondition applies to every key
 * and proof point: they lie in the prime-order subgroups (blsmi_g?_check_batch establishes that).  Under it a block whose equation holds
 * has a failing item with probability at most 2^-64 over the drawn scalars; caller scalars carry 0.17's caveat.
 *   - BLSMI_E_ARG before any device work: a NULL key or proof pointer with m > 0; NULL inputs with m * nin > 0; NULL ok; a zero caller
 *     scalar; m beyond 2^31 - 2 (the pairs A_j, C_j are 32-bit indices; 2^32 - 1 and beyond included); nin beyond 2^20.
 *   - m = 0: BLSMI_OK, *combined = 0.  *rechecked = 0 on every early return.  No `block` value is refused.
 *   - _jac: points as G1Projective / G2Projective records (144 / 288 bytes); _dev: everything but scalars / combined / rechecked resident
 *     on one of the library's devices, `stream` as in blsmi_pairing_batch_dev; the caller's buffers stay untouched.
 * "rlc_min" does NOT apply.  The call takes one lease and runs on one device; it is not split and never joins the request combiner.
 * When to call it (one MI355X, everything resident, block = 0, against the composite a caller had before -- blsmi_g1_mul_batch_dev over m * nin
 * IC records, blsmi_g1_sum_segmented_dev for the L_j, blsmi_pairing_product_batch_rlc_locate_dev -- the two alternating, median of 20 +-
 * spread in ms; DESIGN.md 3t has the table and the stages): for any batch the 0.18 call would serve when the L_j do not exist yet.  All
 * valid, m x nin: 16 384 x 8 11.8 +- 0.1 against 18.4 +- 0.4, 65 536 x 8 23.3 +- 0.4 against 55.7 +- 1.0, 16 384 x 1 10.6 against 15.8; one
 * bad input: 15.8 against 21.5 and 28.5 against 58.3.  The fold itself takes 0.06 ms at 65 536 x 8.  What 0.17 says about a few thousand
 * items or fewer holds here too: 2 048 x 8 takes 6.4 ms (the composite 8.2), behind a per-item check on L_j that already exist. */
int blsmi_groth16_verify_batch(const uint8_t *vk_g1 /* (nin+2)*96 */, const uint8_t *vk_g2 /* 3*192 */, size_t nin, const uint8_t *proof_g1 /* 2m*96 */,
                               const uint8_t *proof_g2 /* m*192 */, const uint8_t *inputs /* m*nin*32 */, size_t m,
                               const uint64_t *scalars /* m, may be NULL */, size_t block /* 0 = automatic */,
                               uint8_t *ok /* m */, int *combined /* may be NULL */, size_t *rechecked /* may be NULL */);
int blsmi_groth16_verify_batch_jac(const uint64_t *vk_g1_jac /* (nin+2)*18 */, const uint64_t *vk_g2_jac /* 3*36 */, size_t nin, const uint64_t *proof_g1_jac /* 2m*18 */,
                                   const uint64_t *proof_g2_jac /* m*36 */, const uint8_t *inputs, size_t m, const uint64_t *scalars, size_t block,
                                   uint8_t *ok, int *combined, size_t *rechecked);
int blsmi_groth16_verify_batch_dev(const void *d_vk_g1, const void *d_vk_g2, size_t nin, const void *d_proof_g1, const void *d_proof_g2, const void *d_inputs, size_t m,
                                   const uint64_t *scalars /* host: m, may be NULL */, size_t block, void *d_ok, int *combined /* host */,
                                   size_t *rechecked /* host */, void *stream);
int blsmi_groth16_verify_batch_jac_dev(const void *d_vk_g1_jac, const void *d_vk_g2_jac, size_t nin, const void *d_proof_g1_jac, const void *d_proof_g2_jac,
                                       const void *d_inputs, size_t m, const uint64_t *scalars, size_t block, void *d_ok, int *combined, size_t *rechecked,
                                       void *stream);

/* ---- the G1 lift and KZG batches (blsmi 0.20) ----------------------------------------------------------------------------------------------
 * out[j] = A_j + (k_j mod r) * B_j in G1, one lane per item in ONE kernel (k_g1_mul_add_glv): the endomorphism ladder of
 * blsmi_g1_mul_batch on B_j, one mixed addition of A_j into its Jacobian result, and the one inversion the ladder pays anyway -- no second
 * launch, no second trip through affine records.  a, b: affine records a_stride / b_stride bytes apart -- 0: one common record; otherwise a
 * multiple of 4 that is at least 96 -- so that points interleaved with other data are read where they lie; scalars: n values of 32
 * big-endian bytes, ANY 256-bit value is taken mod r.  out: n dense records; out_inf[j] = 1 and the all-zero record for a result at infinity.
 * As blsmi_g1_mul_batch, every B_j lies in the prime-order subgroup (blsmi_g1_check_batch establishes that); A_j may be any curve point.
 * The all-zero record is the point at infinity on either side; A_j = k_j * B_j (the addition is a doubling) and A_j = -k_j * B_j are served.
 *   - BLSMI_E_ARG before any device work: a NULL pointer with n > 0, a stride that is neither 0 nor a multiple of 4 from 96 up, n beyond
 *     2^32 - 1.  n = 0: BLSMI_OK.
 *   - _dev: every buffer on one of the library's devices, 4-byte aligned; `stream` as in blsmi_pairing_batch_dev; the inputs stay untouched. */
int blsmi_g1_mul_add_batch(const uint8_t *a /* n records a_stride apart */, size_t a_stride, const uint8_t *b, size_t b_stride,
                           const uint8_t *scalars /* n*32 */, uint8_t *out /* n*96 */, uint8_t *out_inf /* n */, size_t n);
int blsmi_g1_mul_add_batch_dev(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, const void *d_scalars, void *d_out, void *d_out_inf,
                               size_t n, void *stream);
/* m KZG openings under one key, from the commitments, the evaluation points, the values and the proofs themselves: no point
 * P_j = C_j - y_j * G + z_j * pi_j is asked of the caller.  srs_g1: G (1 record); srs_g2: H, tau * H (2 records); commitments: C_j (m
 * records); proofs: pi_j (m records); z, y: m scalars each, 32-byte big-endian, any value taken mod r.  scalars / block / ok / combined /
 * rechecked exactly as blsmi_pairing_product_batch_rlc_locate.
 * Verdicts: ok[j] is exactly is_one[j] of blsmi_pairing_product_batch on the two pairs (P_j, H), (pi_j, -tau * H), with
 * P_j = C_j + (z_j mod r) * pi_j - (y_j mod r) * G.  Infinity (the all-zero affine record, z == 0 in an in-memory record) follows
 * blsmi_pairing_product_batch: the pair contributes 1; an all-zero srs_g2 entry drops its pairs.
 * The path that holds: W_j = C_j + z_j * pi_j by the lift above (one endomorphism ladder per item: z_j differs per item), written straight
 * into the interleaved (W_j, pi_j) array of the two pairs; then per block b of the 0.18 rule (block = 0: max(64, ceil(m / 256))), with the
 * weights r_j,
 *     sum_{j in b} r_j * P_j = sum_{j in b} r_j * W_j - s_b * G,        s_b = sum_{j in b} r_j * y_j mod r
 * -- the 0.19 fold over one column, the blocks as its segments -- so a block costs the two 64-bit weighted sums of 0.18, ONE full-width
 * ladder (s_b over -G; s_b = 0 gives infinity and the cell is left out) and three Miller loops: sum r_j * W_j against H, s_b * (-G) against
 * H, sum r_j * pi_j against -tau * H; the blocks' products, the total and one final exponentiation are those of 0.18.  On this path no
 * y_j * G exists.  When the total fails the block values are final-exponentiated, and for the items of the failing blocks, and only those,
 * P_j is built from the W_j already there (y_j mod r by the fold, one ladder over -G and a two-point sum each; the lift never runs twice) and
 * the two pairs go through blsmi_pairing_product_batch's own path; *rechecked is the number of those items.
 * Soundness: the fold and the lift give the same group elements as the per-item points only for G and pi_j of order r, so 0.17's
 * precondition applies to every key, commitment and proof point: they lie in the prime-order subgroups (blsmi_g?_check_batch establishes
 * that).  Under it a block whose equation holds has a failing item with probability at most 2^-64 over the drawn scalars; caller scalars
 * carry 0.17's caveat.
 *   - BLSMI_E_ARG before any device work: a NULL key, point, scalar-array or ok pointer with m > 0; a zero caller scalar; m beyond
 *     2^31 - 2 (the pairs W_j, pi_j are 32-bit indices; 2^32 - 1 and beyond included).
 *   - m = 0: BLSMI_OK, *combined = 0.  *rechecked = 0 on every early return.  No `block` value is refused.
 *   - _jac: points as G1Projective / G2Projective records (144 / 288 bytes); _dev: everything but scalars / combined / rechecked resident
 *     on one of the library's devices (4-byte aligned), `stream` as in blsmi_pairing_batch_dev; the caller's buffers stay untouched.
 * "rlc_min" does NOT apply.  The call takes one lease and runs on one device; it is not split and never joins the request combiner.
 * When to call it (one MI355X, everything resident, block = 0, against the composite a caller had before -- blsmi_g1_mul_batch_dev for
 * z_j * pi_j and, with d_pts = NULL, for (r - y_j) * G, blsmi_g1_sum_segmented_dev over the three points,
 * blsmi_pairing_product_batch_rlc_locate_dev -- the two alternating, median of 20 +- spread in ms; DESIGN.md 3u has the table and the
 * stages): for any batch the 0.18 call would serve when the P_j do not exist yet.  All valid: 16 384 openings 7.1 +- 0.1 against
 * 10.6 +- 0.6, 65 536 11.9 +- 1.6 against 24.1 +- 0.4; one bad value: 10.8 against 13.1 and 14.4 against 26.6.  What 0.17 says about a few
 * thousand items or fewer holds here too: at 2 048 the call takes 6.5 ms and the composite 5.9. */
int blsmi_kzg_verify_batch(const uint8_t *srs_g1 /* 96 */, const uint8_t *srs_g2 /* 2*192 */, const uint8_t *commitments /* m*96 */,
                           const uint8_t *proofs /* m*96 */, const uint8_t *z /* m*32 */, const uint8_t *y /* m*32 */, size_t m,
                           const uint64_t *scalars /* m, may be NULL */, size_t block /* 0 = automatic */,
                           uint8_t *ok /* m */, int *combined /* may be NULL */, size_t *rechecked /* may be NULL */);
int blsmi_kzg_verify_batch_jac(const uint64_t *srs_g1_jac /* 18 */, const uint64_t *srs_g2_jac /* 2*36 */, const uint64_t *commitments_jac /* m*18 */,
                               const uint64_t *proofs_jac /* m*18 */, const uint8_t *z, const uint8_t *y, size_t m, const uint64_t *scalars, size_t block,
                               uint8_t *ok, int *combined, size_t *rechecked);
int blsmi_kzg_verify_batch_dev(const void *d_srs_g1, const void *d_srs_g2, const void *d_commitments, const void *d_proofs, const void *d_z, const void *d_y, size_t m,
                               const uint64_t *scalars /* host: m, may be NULL */, size_t block, void *d_ok, int *combined /* host */,
                               size_t *rechecked /* host */, void *stream);
int blsmi_kzg_verify_batch_jac_dev(const void *d_srs_g1_jac, const void *d_srs_g2_jac, const void *d_commitments_jac, const void *d_proofs_jac,
                                   const void *d_z, const void *d_y, size_t m, const uint64_t *scalars, size_t block, void *d_ok, int *combined, size_t *rechecked,
                                   void *stream);

/* ---- polynomial evaluation in Fr and KZG blob batches (blsmi 0.21) ---------------------------------------------------------------------------
 * The scalar field proper on the device: Montgomery products and inverses mod r (the order of G1, G2 and GT), a lane per element.
 * a, b, out: n scalars of 32 big-endian bytes; ANY 256-bit value is taken mod r, every output is fully reduced; the inverse of 0 mod r
 * (0, r, 2 r) is 0.
 *   - BLSMI_E_ARG before any device work: a NULL pointer with n > 0, n beyond 2^32 - 1.  n = 0: BLSMI_OK, nothing is written.
 *   - _dev: every buffer on one of the library's devices, 4-byte aligned; `stream` as in blsmi_pairing_batch_dev; the inputs stay untouched
 *     (out may be an input's buffer: a lane reads its element before it writes it). */
int blsmi_fr_mul_batch(const uint8_t *a /* n*32 */, const uint8_t *b /* n*32 */, uint8_t *out /* n*32 */, size_t n);
int blsmi_fr_mul_batch_dev(const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int blsmi_fr_inv_batch(const uint8_t *a /* n*32 */, uint8_t *out /* n*32 */, size_t n);
int blsmi_fr_inv_batch_dev(const void *d_a, void *d_out, size_t n, void *stream);
/* y[j] = p_j(z_j) for m polynomials in EVALUATION form: polynomial j is its N = 2^log2n values over the N-th roots of unity, 32 big-endian
 * bytes each, log2n <= 16.  The domain is w^0 .. w^(N-1), w = 7^((r - 1) / N) mod r (log2n = 12: 0x564c0a11...a5d36306, the root of
 * EIP-4844).  order = 0: the value at position i belongs to w^i; order = 1: to w^bitrev(i), i's log2n bits reversed -- the layout of a
 * blob.  z: m points; y: m values, fully reduced.  ANY 256-bit value or point is taken mod r like every scalar of the library;
 * noncanon (may be NULL): noncanon[j] = 1 when any of polynomial j's N values was >= r, else 0 -- for the caller to reject.
 * By the barycentric formula p(z) = (z^N - 1) / N * sum_i f_i w_i / (z - w_i), one workgroup per polynomial and ONE inversion per
 * polynomial, in three launches: k_fr_bary_prod (the product of the z - w_i), k_fr_inv, k_fr_bary_sum.  Where z_j is a root of the domain
 * (after reduction: w_i + r is w_i) the answer is the value at that position mod r, read directly.
 * The domain's table (N + 1 elements, 32 bytes each) is built once per (device, log2n, order) at the first call that needs it and kept
 * until blsmi_shutdown: it is a per-device constant, so blsmi_trim does not release it and blsmi_held_bytes does not count it.
 *   - BLSMI_E_ARG before any device work: NULL polys, z or y with m > 0; log2n > 16; order neither 0 nor 1; m beyond 2^32 - 1; m * N * 32
 *     beyond a size_t.  m = 0: BLSMI_OK, nothing is written.
 *   - _dev: every buffer on one of the library's devices, 4-byte aligned (polys is read in 16-byte pieces when it is 16-byte aligned, byte
 *     by byte otherwise); `stream` as in blsmi_pairing_batch_dev; the inputs stay untouched.
 * One lease, one device, never in the request combiner. */
int blsmi_fr_eval_batch(const uint8_t *polys /* m*N*32 */, unsigned log2n, int order, const uint8_t *z /* m*32 */, uint8_t *y /* m*32 */,
                        uint8_t *noncanon /* m, may be NULL */, size_t m);
int blsmi_fr_eval_batch_dev(const void *d_polys, unsigned log2n, int order, const void *d_z, void *d_y, void *d_noncanon /* may be NULL */, size_t m,
                            void *stream);
/* m KZG blob proofs under one key: blsmi_kzg_verify_batch for a caller who holds the polynomial and not its value.  polys / log2n / order as
 * blsmi_fr_eval_batch; srs_g1, srs_g2, commitments, proofs, z, scalars / block / ok / combined / rechecked exactly as blsmi_kzg_verify_batch.
 * y_j = p_j(z_j) is computed by the evaluation above into the call's own buffer; everything after that IS blsmi_kzg_verify_batch:
 * ok[j] is exactly its verdict on (C_j, pi_j, z_j, p_j(z_j)), with its infinity rules, its block equations, its recheck and its
 * soundness precondition (every key, commitment and proof point in the prime-order subgroups).  A non-canonical value is taken mod r; it is
 * reported in noncanon (may be NULL) as blsmi_fr_eval_batch reports it, for the caller to reject -- ok[j] does not depend on it.
 * Deriving z_j by Fiat-Shamir (SHA-256 over the blob and the commitment, EIP-4844's compute_challenge) stays the caller's: z is an input
 * HERE.  blsmi_kzg_verify_blob_batch_wire (0.23, below) derives it on the device, from the bytes a caller of the EIP function holds.
 *   - BLSMI_E_ARG before any device work: a NULL key, polys, point, z or ok pointer with m > 0; log2n > 16; order neither 0 nor 1; a zero
 *     caller scalar; m beyond 2^31 - 2 (2^32 - 1 and beyond included); m * N * 32 beyond a size_t.
 *   - m = 0: BLSMI_OK, *combined = 0, nothing else is written.  *rechecked = 0 on every early return.  No `block` value is refused.
 *   - _jac / _dev as blsmi_kzg_verify_batch; polys, z, ok and noncanon are then device buffers, 4-byte aligned; the caller's buffers stay
 *     untouched.
 * "rlc_min" does NOT apply.  The call takes one lease and runs on one device; it is not split and never joins the request combiner.
 * What it does not change: the floor of 0.17 (a call costs a few milliseconds whatever m) and the lift of 0.20 (one ladder per item)
 * remain under it -- the evaluation is added in front of blsmi_kzg_verify_batch, nothing of that call is removed or made cheaper.
 * Measured (one MI355X, everything resident, N = 4 096, block = 0, the legs alternating, median of 20 +- spread in ms; DESIGN.md 3v and
 * profiles/r21_blob_eval.log have the table): (a) the evaluation, its three kernels
 * in brackets (k_fr_bary_prod, k_fr_inv, k_fr_bary_sum); (b) a device-to-device copy of the same m * N * 32 bytes; (c)
 * blsmi_kzg_verify_batch_dev on the same openings with y given; (d) this call.
 *     m = 8:      (a) 0.71 +- 0.17 (0.04, 0.51, 0.14)   (b) 0.02   (a) / (b) 32    (c) 6.16 +- 0.27   (d) 6.80 +- 0.22   (d) - (c) 0.64
 *     m = 64:     (a) 0.65 +- 0.01 (0.04, 0.45, 0.14)   (b) 0.03   (a) / (b) 26    (c) 6.32 +- 0.02   (d) 6.88 +- 0.04   (d) - (c) 0.56
 *     m = 1 024:  (a) 0.93 +- 0.03 (0.10, 0.45, 0.36)   (b) 0.05   (a) / (b) 17    (c) 6.49 +- 0.13   (d) 7.39 +- 0.08   (d) - (c) 0.90
 *     m = 4 096:  (a) 2.01 +- 0.02 (0.31, 0.46, 1.21)   (b) 0.21   (a) / (b) 9.8   (c) 6.90 +- 0.08   (d) 8.87 +- 0.08   (d) - (c) 1.97
 * The evaluation is bound by the multiplier, not by HBM (9.8 times the copy at 512 MB of blobs), and up to a thousand blobs by the one
 * inversion's latency (k_fr_inv: 0.45 ms for one element as for 65 536).  At NONE of the measured m is the evaluation the larger part of the
 * call: at 4 096 blobs the pairings' side -- the lift, the sums, three Miller loops per block, the final exponentiation -- still takes 3.4
 * times as long, and up to a thousand blobs seven to ten times. */
int blsmi_kzg_verify_blob_batch(const uint8_t *srs_g1 /* 96 */, const uint8_t *srs_g2 /* 2*192 */, const uint8_t *polys /* m*N*32 */, unsigned log2n, int order,
                                const uint8_t *commitments /* m*96 */, const uint8_t *proofs /* m*96 */, const uint8_t *z /* m*32 */, size_t m,
                                const uint64_t *scalars /* m, may be NULL */, size_t block /* 0 = automatic */, uint8_t *ok /* m */,
                                uint8_t *noncanon /* m, may be NULL */, int *combined /* may be NULL */, size_t *rechecked /* may be NULL */);
int blsmi_kzg_verify_blob_batch_jac(const uint64_t *srs_g1_jac /* 18 */, const uint64_t *srs_g2_jac /* 2*36 */, const uint8_t *polys, unsigned log2n, int order,
                                    const uint64_t *commitments_jac /* m*18 */, const uint64_t *proofs_jac /* m*18 */, const uint8_t *z, size_t m,
                                    const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *noncanon, int *combined, size_t *rechecked);
int blsmi_kzg_verify_blob_batch_dev(const void *d_srs_g1, const void *d_srs_g2, const void *d_polys, unsigned log2n, int order, const void *d_commitments,
                                    const void *d_proofs, const void *d_z, size_t m, const uint64_t *scalars /* host: m, may be NULL */, size_t block,
                                    void *d_ok, void *d_noncanon /* may be NULL */, int *combined /* host */, size_t *rechecked /* host */, void *stream);
int blsmi_kzg_verify_blob_batch_jac_dev(const void *d_srs_g1_jac, const void *d_srs_g2_jac, const void *d_polys, unsigned log2n, int order,
                                        const void *d_commitments_jac, const void *d_proofs_jac, const void *d_z, size_t m, const uint64_t *scalars, size_t block,
                                        void *d_ok, void *d_noncanon, int *combined, size_t *rechecked, void *stream);

/* ==== coset interpolation in Fr and KZG cell batches (blsmi 0.22) ==============================================================================
 * coeffs[j] = the n = 2^log2n coefficients of the polynomial I_j with deg I_j < n that takes the values vals[j] over the COSET h_j <w>:
 * w = 7^((r - 1) / n) mod r, the root of the domains of blsmi_fr_eval_batch; order = 0: the value at position i belongs to h_j w^i;
 * order = 1: to h_j w^bitrev(i), i's log2n bits reversed -- a cell of EIP-7594 as it arrives (n = 64, h_k = w_8192^bitrev_7(k) for cell k).
 * vals: n values per item, 32 big-endian bytes each; shifts: the m values h_j.  ANY 256-bit value or shift is taken mod r like every scalar
 * of the library.  coeffs[j][i] is the coefficient of X^i: natural order, fully reduced.  shift_pow (may be NULL): shift_pow[j] = h_j^n mod r.
 * flags (may be NULL): bit 0 of flags[j] is set when a value or the shift of item j was >= r, bit 1 when h_j = 0 mod r -- for the caller to
 * reject.  h_j = 0 mod r is NOT refused: no coset exists then, and the formula runs with 0^-1 = 0 (as blsmi_fr_inv_batch) and 0^0 = 1, so
 * that c_j0 = a_j0 and c_ji = 0 for i > 0; the caller rejects by the flag.
 * With a_j the inverse DFT of the values over w, the factor 1 / n included, c_ji = h_j^(-i) a_ji.  Two launches: k_fr_inv over the m shifts,
 * then k_fr_coset_interp: a workgroup holds 512 / n items in LDS (n = 1 024: one), log2n stages of butterflies, a scaling by the powers of
 * h_j^-1.  The twiddles are the order-0 domain table of blsmi_fr_eval_batch of size n, kept until blsmi_shutdown as that call says.
 *   - log2n <= 10.
 *   - BLSMI_E_ARG before any device work: NULL vals, shifts or coeffs with m > 0; log2n > 10; order neither 0 nor 1; m beyond 2^32 - 1;
 *     m * n * 32 beyond a size_t.  m = 0: BLSMI_OK, nothing is written.
 *   - coeffs must not overlap vals: a workgroup reads all of its items before it writes any, but several items share a workgroup and
 *     workgroups do not wait for each other.
 *   - _dev: every buffer on one of the library's devices, 4-byte aligned (vals is read in 16-byte pieces when it is 16-byte aligned, byte by
 *     byte otherwise); `stream` as in blsmi_pairing_batch_dev; the inputs stay untouched.
 * One lease, one device, never in the request combiner. */
int blsmi_fr_coset_interp_batch(const uint8_t *vals /* m*n*32 */, unsigned log2n, int order, const uint8_t *shifts /* m*32 */, uint8_t *coeffs /* m*n*32 */,
                                uint8_t *shift_pow /* m*32, may be NULL */, uint8_t *flags /* m, may be NULL */, size_t m);
int blsmi_fr_coset_interp_batch_dev(const void *d_vals, unsigned log2n, int order, const void *d_shifts, void *d_coeffs, void *d_shift_pow /* may be NULL */,
                                    void *d_flags /* may be NULL */, size_t m, void *stream);
/* m KZG cell proofs under one key: cell j is the n = 2^log2n values of the polynomial committed to by C_j over the coset h_j <w>, with ONE
 * proof pi_j for all of them (EIP-7594: n = 64, order = 1).  vals / log2n / order / shifts as blsmi_fr_coset_interp_batch; srs_g1: the key's
 * [tau^0] G .. [tau^(n-1)] G; srs_g2: H and [tau^n] H; scalars / block / ok / combined / rechecked exactly as blsmi_kzg_verify_batch.
 * The cell holds when e(C_j - [I_j(tau)] G, H) = e(pi_j, [tau^n - h_j^n] H).  ok[j] is exactly is_one[j] of blsmi_pairing_product_batch on
 * (P_j, H), (pi_j, -[tau^n] H) with
 *     P_j = C_j + (h_j^n mod r) pi_j - sum_i c_ji [tau^i] G,        c_j the coefficients blsmi_fr_coset_interp_batch gives,
 * with the infinity rules, the block equations, the recheck and the soundness precondition (every key, commitment and proof point in the
 * prime-order subgroups) of blsmi_kzg_verify_batch: this is that call's equation with z_j := h_j^n, y_j G := sum_i c_ji [tau^i] G and
 * tau H := [tau^n] H.  Over a block the coefficients are folded first, s_bi = sum_j r_j c_ji mod r, so that a block costs n full-width
 * ladders over the negated key records and one segmented sum, whatever its length; no [I_j(tau)] G exists on the path that holds.
 * flags (may be NULL) as blsmi_fr_coset_interp_batch reports them, for the caller to reject -- ok[j] does not depend on them.
 *   - BLSMI_E_ARG before any device work: a NULL key, vals, shifts, point or ok pointer with m > 0; log2n > 10; order neither 0 nor 1; a zero
 *     caller scalar; m beyond 2^31 - 2 (2^32 - 1 and beyond included); m * n * 32 beyond a size_t.
 *   - m = 0: BLSMI_OK, *combined = 0, nothing else is written.  *rechecked = 0 on every early return.  No `block` value is refused.
 *   - _jac / _dev as blsmi_kzg_verify_batch; vals, shifts, ok and flags are then device buffers, 4-byte aligned; the caller's buffers stay
 *     untouched.
 * "rlc_min" does NOT apply.  The call takes one lease and runs on one device; it is not split and never joins the request combiner.
 * What it does not change: the floor of 0.17 and the lift of 0.20 remain under it -- the interpolation, the n-column fold and B * n ladders
 * (B blocks) are added to blsmi_kzg_verify_batch's work, nothing of that call is removed or made cheaper.
 * Measured (one MI355X, everything resident, n = 64, order 1, block = 0, the legs alternating, median of 20 +- spread in ms; DESIGN.md 3w and
 * profiles/r22_cell.log have the table): (a) the interpolation, its two kernels in brackets (k_fr_inv, k_fr_coset_interp); (b) a
 * device-to-device copy of the same m * n * 32 bytes; (c) blsmi_kzg_verify_batch_dev on m openings over the same key points; (d) this call,
 * every cell valid; (e) this call with one value spoiled (a block of 64 cells is rechecked).
 *     m = 128:     (a) 0.52 +- 0.15 (0.45, 0.05)   (b) 0.02   (a) / (b) 22   (c) 6.21 +- 0.23   (d)  7.14 +- 0.11   (d) - (c) 0.93   (e) 12.57 +- 0.20
 *     m = 1 024:   (a) 0.52 +- 0.16 (0.45, 0.06)   (b) 0.03   (a) / (b) 21   (c) 6.44 +- 0.16   (d)  7.43 +- 0.11   (d) - (c) 0.99   (e) 12.92 +- 0.32
 *     m = 8 192:   (a) 0.61 +- 0.01 (0.45, 0.15)   (b) 0.03   (a) / (b) 24   (c) 6.70 +- 0.08   (d) 11.74 +- 0.16   (d) - (c) 5.04   (e) 17.13 +- 0.19
 *     m = 16 384:  (a) 0.76 +- 0.02 (0.46, 0.29)   (b) 0.03   (a) / (b) 24   (c) 7.16 +- 0.25   (d)  9.77 +- 0.10   (d) - (c) 2.62   (e) 15.27 +- 0.10
 * The interpolation is bound by the one inversion's latency (k_fr_inv: 0.45 ms for 128 shifts as for 16 384), not by HBM.  The B * n key
 * ladders are the largest single addition but never more than the rest of the call: 0.8 ms up to 1 024 cells, 2.2 ms of 9.8 at 16 384 (256
 * blocks, 16 384 ladders, k_g1_mul_glv), and 4.8 ms of 11.7 at 8 192 -- 8 192 ladders are the most that the wave-per-scalar ladder of small
 * calls still takes (k_lat:mul1), so that 8 192 cells cost MORE than 16 384.  One spoiled value costs 5.4 ms whatever m: 64 cells are
 * rechecked with 64 ladders each. */
int blsmi_kzg_verify_cell_batch(const uint8_t *srs_g1 /* n*96: [tau^0]G .. [tau^(n-1)]G */, const uint8_t *srs_g2 /* 2*192: H, [tau^n]H */,
                                const uint8_t *vals /* m*n*32 */, unsigned log2n, int order, const uint8_t *shifts /* m*32 */,
                                const uint8_t *commitments /* m*96 */, const uint8_t *proofs /* m*96 */, size_t m,
                                const uint64_t *scalars /* m, may be NULL */, size_t block /* 0 = automatic */, uint8_t *ok /* m */,
                                uint8_t *flags /* m, may be NULL */, int *combined /* may be NULL */, size_t *rechecked /* may be NULL */);
int blsmi_kzg_verify_cell_batch_jac(const uint64_t *srs_g1_jac /* n*18 */, const uint64_t *srs_g2_jac /* 2*36 */, const uint8_t *vals, unsigned log2n, int order,
                                    const uint8_t *shifts, const uint64_t *commitments_jac /* m*18 */, const uint64_t *proofs_jac /* m*18 */, size_t m,
                                    const uint64_t *scalars, size_t block, uint8_t *ok, uint8_t *flags, int *combined, size_t *rechecked);
int blsmi_kzg_verify_cell_batch_dev(const void *d_srs_g1, const void *d_srs_g2, const void *d_vals, unsigned log2n, int order, const void *d_shifts,
                                    const void *d_commitments, const void *d_proofs, size_t m, const uint64_t *scalars /* host: m, may be NULL */, size_t block,
                                    void *d_ok, void *d_flags /* may be NULL */, int *combined /* host */, size_t *rechecked /* host */, void *stream);
int blsmi_kzg_verify_cell_batch_jac_dev(const void *d_srs_g1_jac, const void *d_srs_g2_jac, const void *d_vals, unsigned log2n, int order, const void *d_shifts,
                                        const void *d_commitments_jac, const void *d_proofs_jac, size_t m, const uint64_t *scalars, size_t block,
                                        void *d_ok, void *d_flags, int *combined, size_t *rechecked, void *stream);

/* ==== Fiat-Shamir challenge and KZG blob batches from wire bytes (blsmi 0.23) ==================================================================
 * z[j] = SHA-256(D_j) mod r as 32 big-endian bytes, fully reduced, with
 *     D_j = "FSBLOBVERIFY_V1_" || N as 16 big-endian bytes || blob_j as it lies || commitment_j as it lies,        N = 2^log2n,
 * EIP-4844's compute_challenge.  polys: m blobs of N values of 32 bytes; commitments48: m compressed commitments of 48 bytes.  The bytes are
 * hashed AS THEY ARE: nothing is decoded, reduced or validated here, so a non-canonical value or an undecodable commitment changes only the
 * digest.  The digest can be >= r and >= 2 r: up to two subtractions.  D_j is 32 N + 80 bytes, N / 2 + 2 compression blocks (N = 1: 2); the
 * blocks are built from word loads (bls_amd/csrc/sha256_fs.h has the layout), 16-byte loads where a block lies whole in a 16-byte aligned
 * blob.  One launch of k_kzg_fs_split: a workgroup of two waves serves 64 blobs, one wave on the message schedule of block i + 1 while the
 * other runs the rounds of block i (k_kzg_fs_lane, one lane per blob doing both, is kept for comparison behind
 * blsmi_debug_kzg_blob_challenge_form_dev, form 0; form 1 is the default; any other form: BLSMI_E_ARG).
 *   - log2n <= 16.
 *   - BLSMI_E_ARG before any device work: NULL polys, commitments48 or z with m > 0; log2n > 16; m beyond 2^32 - 1; m * N * 32 beyond a
 *     size_t.  m = 0: BLSMI_OK, nothing is written.
 *   - _dev: every buffer on one of the library's devices, 4-byte aligned; `stream` as in blsmi_pairing_batch_dev; the inputs stay untouched.
 * One lease, one device, never in the request combiner. */
int blsmi_kzg_blob_challenge_batch(const uint8_t *polys /* m*N*32 */, unsigned log2n, const uint8_t *commitments48 /* m*48 */, uint8_t *z /* m*32 */, size_t m);
int blsmi_kzg_blob_challenge_batch_dev(const void *d_polys, unsigned log2n, const void *d_commitments48, void *d_z, size_t m, void *stream);
int blsmi_debug_kzg_blob_challenge_form_dev(const void *d_polys, unsigned log2n, const void *d_commitments48, void *d_z, size_t m, int form /* 0: k_kzg_fs_lane, 1: k_kzg_fs_split */,
                                            void *stream);
/* EIP-4844's verify_blob_kzg_proof_batch: m blob proofs under one key from the three byte strings a caller of that function holds per item
 * -- the blob (N = 2^log2n values of 32 big-endian bytes in the blob's own, bit-reversed order: order = 1 of blsmi_fr_eval_batch, not a
 * parameter), the 48-byte compressed commitment, the 48-byte compressed proof.  srs_g1, srs_g2, scalars / block / combined / rechecked as
 * blsmi_kzg_verify_blob_batch (the key is its affine records).  Stages, the buffers being the call's own:
 *     1  z_j by blsmi_kzg_blob_challenge_batch_dev
 *     2  beside it, on the lease's side stream, ONE k_g1_decompress launch over the 2 m compressed points with the subgroup test
 *        (check = 1 of blsmi_g1_decompress_batch), into AFFINE records: the form the lift of 0.20 reads, no further pass
 *     3  y_j = p_j(z_j) by blsmi_fr_eval_batch_dev, with noncanon
 *     4  blsmi_kzg_verify_batch_dev's check, unchanged
 * status (may be NULL): status[j] = errC | errPi << 3 | noncanon << 6, errC and errPi the codes of blsmi_g1_decompress_batch (0 .. 4) for the
 * commitment and the proof, noncanon as blsmi_fr_eval_batch reports it.  ok[j] = 1 EXACTLY when status[j] == 0 and blsmi_kzg_verify_batch's
 * verdict on (C_j, pi_j, z_j, p_j(z_j)) is 1.  A well-formed infinity (0xc0, then zeros) is a VALID point, as in the EIP: the zero blob with
 * C = pi = infinity has ok = 1.  A point that does not decode is never taken for infinity: the zero blob with 48 bytes of 0xff for both points
 * has ok = 0.  A value >= r is rejected (status 0x40) although z_j and a proof made for it may hold mod r.
 * An item with status != 0 is CLEARED before stage 4 -- both points to infinity, y_j to 0: the item that holds trivially -- so that it fails
 * no block: *combined = 1 exactly when the combined check over the items with status 0 held (then ok[j] = (status[j] == 0) for every j),
 * and *rechecked counts the items, cleared ones included, of the blocks in which an item with status 0 fails, as blsmi_kzg_verify_batch counts
 * them.  A caller who wants "the whole batch is valid" tests *combined AND every status byte, or every ok byte.
 *   - BLSMI_E_ARG before any device work: a NULL key, polys, point or ok pointer with m > 0; log2n > 16; a zero caller scalar; m beyond
 *     2^31 - 2 (2^32 - 1 and beyond included); m * N * 32 beyond a size_t.
 *   - m = 0: BLSMI_OK, *combined = 0, nothing else is written.  *rechecked = 0 on every early return.  No `block` value is refused.
 *   - _dev: every buffer but scalars, combined and rechecked on one of the library's devices, 4-byte aligned; `stream` as in
 *     blsmi_pairing_batch_dev; the caller's buffers stay untouched.  blsmi_debug_kzg_verify_blob_batch_wire_dev_serial is the same call
 *     with stage 2 on the main stream, in front of stage 1: the leg the overlap is measured against.
 * "rlc_min" does NOT apply.  The call takes one lease and runs on one device; it is not split and never joins the request combiner.
 * What it does not change: blsmi_kzg_verify_blob_batch and everything under it -- the floor of 0.17, the lift of 0.20, the evaluation of
 * 0.21 -- stay as they are; the hash, the decompression and two byte kernels are added in front.  There is no Go shim and no multi-device
 * split for these calls.
 * Measured (one MI355X, everything resident, N = 4 096, block = 0, every item valid, median of 20 +- spread in ms; DESIGN.md 3x and
 * profiles/r23_blob_wire.log have the tables): (a) the challenge, k_kzg_fs_split; (A) the same by k_kzg_fs_lane, the two alternating; (b) a
 * device-to-device copy of the same m * N * 32 bytes; (h) hashlib.sha256 over the same blobs on 1 / 16 host threads; (c)
 * blsmi_kzg_verify_blob_batch_dev given z and the affine points; (d) this call; (e) its _serial twin.
 *     m = 8:      (a) 4.10 +- 0.03   (A) 7.39 +- 0.24   (b) 0.02   (h) 0.46 / 0.41    (c) 6.85 +- 0.31   (d) 11.04 +- 0.48   (e) 12.64 +- 0.47
 *     m = 64:     (a) 4.11 +- 0.03   (A) 7.84 +- 0.05   (b) 0.03   (h) 3.67 / 2.78    (c) 6.86 +- 0.20   (d) 11.07 +- 0.05   (e) 12.69 +- 0.07
 *     m = 1 024:  (a) 4.16 +- 0.03   (A) 7.88 +- 0.04   (b) 0.15   (h) 61.4 / 34.7    (c) 7.38 +- 0.43   (d) 12.50 +- 1.19   (e) 13.19 +- 0.07
 *     m = 4 096:  (a) 4.23 +- 0.02   (A) 8.11 +- 0.03   (b) 0.32   (h) 241 / 147      (c) 8.87 +- 0.17   (d) 14.28 +- 1.14   (e) 14.77 +- 0.13
 * The challenge has a floor of 4.1 ms whatever m: one blob is 2 050 dependent compressions and a wave costs the same with one lane as with 64.
 * BELOW ABOUT 70 BLOBS THE HOST'S HASH IS THE BETTER CHOICE (8 blobs: 0.46 ms on one thread); from a few hundred blobs the device is, 57
 * times at 4 096.  (d) - (c), what the wire call adds, is 4.2 to 5.4 ms; the side stream saves 1.6 ms up to 64 blobs and is never slower
 * beyond the spread. */
int blsmi_kzg_verify_blob_batch_wire(const uint8_t *srs_g1 /* 96 */, const uint8_t *srs_g2 /* 2*192 */, const uint8_t *polys /* m*N*32 */, unsigned log2n,
                                     const uint8_t *commitments48 /* m*48 */, const uint8_t *proofs48 /* m*48 */, size_t m,
                                     const uint64_t *scalars /* m, may be NULL */, size_t block /* 0 = automatic */, uint8_t *ok /* m */,
                                     uint8_t *status /* m, may be NULL */, int *combined /* may be NULL */, size_t *rechecked /* may be NULL */);
int blsmi_kzg_verify_blob_batch_wire_dev(const void *d_srs_g1, const void *d_srs_g2, const void *d_polys, unsigned log2n, const void *d_commitments48,
                                         const void *d_proofs48, size_t m, const uint64_t *scalars /* host: m, may be NULL */, size_t block, void *d_ok,
                                         void *d_status /* may be NULL */, int *combined /* host */, size_t *rechecked /* host */, void *stream);
int blsmi_debug_kzg_verify_blob_batch_wire_dev_serial(const void *d_srs_g1, const void *d_srs_g2, const void *d_polys, unsigned log2n, const void *d_commitments48,
                                                      const void *d_proofs48, size_t m, const uint64_t *scalars, size_t block, void *d_ok, void *d_status,
                                                      int *combined, size_t *rechecked, void *stream);

#ifdef __cplusplus
}
#endif
#endif
