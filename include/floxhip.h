/* floxhip — MI355X (gfx950) grouped-reduction engine: C ABI.
 *
 * This is the drop-in boundary for the hot path of xarray-contrib/flox
 * (reference: flox/core.py:214-394 `chunk_reduce` and the per-engine
 * aggregate modules flox/aggregate_flox.py / flox/aggregate_npg.py).
 * The Python shim flox_amd/aggregate_hip.py implements the reference's
 * engine-plugin interface (flox/aggregations.py:60-133 `generic_aggregate`:
 * one callable per reduction name, signature
 * f(group_idx, array, *, axis=-1, size=None, fill_value=None, dtype=None))
 * on top of exactly these entry points.
 *
 * One call = one fused factorize+reduce pass over `n` rows producing
 * per-group partial bins (the "intermediates" of the reference's
 * IntermediateDict, flox/types.py:28). Multi-GPU combine = an RCCL
 * all-reduce of these bins, applying the reference's combine recipes
 * (flox/aggregations.py:304-546).
 *
 * All pointers are DEVICE pointers; the caller owns every buffer and
 * synchronises via `stream` (a hipStream_t). Calls are stateless and
 * thread-safe. Errors: non-zero return, message via fh_error_string().
 */
#ifndef FLOXHIP_H
#define FLOXHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* value dtypes */
enum fh_dtype { FH_F32 = 0, FH_F64 = 1, FH_I64 = 2, FH_I32 = 3 };
/* label dtypes */
enum fh_ldtype {
  FH_L_I64 = 0,
  FH_L_I32 = 1,
  /* precomputed compact codes (the label-code cache): a u16 label IS the
   * final group code, also for 2-D groupbys (labels2 must be NULL), and
   * 0xFFFF means "in no group" — the unsigned bounds check drops it, since
   * ngroups stays below 65535 wherever the bins fit LDS. Valid only where
   * the LDS-binned path is taken (fh_query_path() == 1); any other dispatch
   * returns error 12. */
  FH_L_U16 = 2,
  /* the same codes packed to 12 / 14 bits in 1024-row tiles
   * (include/floxhip_codes.h; written by fh_pack_codes): `labels` points at
   * fh_packed_code_bytes(n, W) bytes, the all-ones W-bit value means "in no
   * group", and ngroups must stay below it (<= 4094 / <= 16382). Same
   * conditions and error 12 as FH_L_U16. Neither fh_query_path nor
   * fh_scratch_bytes depends on the label dtype. */
  FH_L_P12 = 3,
  FH_L_P14 = 4,
};

/* Fused op sets: the per-group partials one pass produces.
 * (SUM accumulates float inputs in float64 — the numpy_groupies numerics
 * contract pinned by reference tests/test_properties.py:146-151.) */
enum fh_opset {
  FH_SET_SUM_COUNT = 0,         /* sum(f64/i64) + count(i64): mean, var pass 1 */
  FH_SET_SUM_COUNT_PRESENT = 1, /* + per-group "any row seen" flag: sum/nansum */
  FH_SET_COUNT = 2,             /* count only */
  FH_SET_MIN_FULL = 3,          /* min + count + present + nanflag: min */
  FH_SET_MIN_COUNT = 4,         /* min + count: nanmin */
  FH_SET_MAX_FULL = 5,          /* max + count + present + nanflag: max */
  FH_SET_MAX_COUNT = 6,         /* max + count: nanmax */
  FH_SET_SSD = 7,               /* sum of (x - mean[g])^2, f64: var pass 2 */
  FH_SET_PROD = 8,              /* product + count + present (CAS loop) */
  /* index extremum + count + present: the second pass of arg-reductions
   * (reference chunk_argreduce core.py:157-211 / argmax-argmin recipes
   * aggregations.py:582-649) and of first/last/nanfirst/nanlast. With
   * `target` set, only rows whose value equals target[group] (NaN matches
   * NaN) are candidates; without it every (valid, and non-NaN when
   * FH_SKIPNAN) row is. IDXMIN keeps the smallest row index, IDXMAX the
   * largest; out_count/out_present as usual; the index (+ row_offset, for
   * multi-GPU shards) lands in out_sum as int64, -2^63.. sentinel for
   * untouched groups handled by init (IDXMIN: INT64_MAX, IDXMAX: -1).
   * fh_grouped_reduce_cols serves both sets without `target` (error 19 with
   * one): per (group, column) the smallest / largest original row perm[i]
   * (+ row_offset) among the group's rows, the non-NaN ones under
   * FH_SKIPNAN; out_sum is int64 (ngroups, m) with the same sentinels, and
   * out_count / out_present mean what they mean in 1-D: non-NaN rows, any
   * row seen. */
  FH_SET_IDXMIN = 9,
  FH_SET_IDXMAX = 10,
  /* single-pass variance partials for the COLUMN path only: per (group,
   * column) the kernel accumulates shifted sums about the segment's first
   * value (the stability device numpy_groupies also uses,
   * aggregate_npg.py:112-126) and emits the var_chunk triple of the
   * reference (aggregations.py:348-389): ssd -> out_sum (f64),
   * sum -> out_min (f64, pointer reused), count -> out_count. */
  FH_SET_WELFORD = 11,
  /* single-call arg-reductions for 8-byte value dtypes (f64/i64) at group
   * counts beyond the LDS IDX bins, where no 32-bit value encoding can
   * pack into one int64 key: the partition pairs carry the row index in
   * their spare pad word, phase 1 is the ordinary bucketed MIN/MAX (+count
   * +present +nanflag), and a second bucket pass (k_reduce_bucket_argrow)
   * re-reads the SCATTERED pairs and takes the smallest row whose value
   * equals the group's extremum — target lookups are LDS-local after the
   * partition, unlike the two-pass form's random 80 MB gathers. Requires
   * the partition path (returns error 11 otherwise); rows must satisfy
   * row_offset + n < 2^32. Outputs: out_sum = int64 row index (INT64_MAX
   * for empty; first occurrence on ties, np.argmin semantics),
   * out_min/out_max = the decoded extremum, plus count/present/nanflag. */
  FH_SET_ARGMIN_PAIR = 12,
  FH_SET_ARGMAX_PAIR = 13,
  /* every partial the sum/mean/var/std/min/max/count family (and its nan*
   * twins) needs, from ONE pass on the LDS-binned path or on the column
   * path. NaN rows contribute
   * nothing to any member but nanflag (FH_SKIPNAN is implied), so the
   * non-skipping functions are derived by the caller: NaN where nanflag is
   * set. Outputs: out_sum (f64 / i64, as FH_SET_SUM_COUNT), out_count (non-NaN
   * rows), out_min / out_max (value dtype, +inf/-inf or INT_MAX/MIN where
   * count == 0), out_nanflag, out_present (count > 0 || nanflag, i.e. "any
   * row seen") and out_ssd: f64 sum of squared deviations about the group
   * mean. The second moment needs no input from the caller: each workgroup
   * keeps, per group, a pivot x0 (a value it saw for the group) with
   * s1 = sum(x - x0) and s2 = sum((x - x0)^2) in f64, flushes the triple
   * (n_b, mean_b = x0 + s1/n_b, M2_b = s2 - s1^2/n_b), the mean kept as its
   * two parts so that differences of means stay exact, and the combine folds
   * the triples in a fixed order with Chan's pairwise merge
   * M2 = M2_a + M2_b + d^2 n_a n_b / (n_a + n_b), d = mean_b - mean_a.
   * fh_grouped_reduce serves the set on the LDS-binned path only
   * (fh_query_path() == 1): any other dispatch returns error 15 without
   * launching. fh_grouped_reduce_cols serves it at any group count, outputs
   * (ngroups, m): each thread keeps the same state per column in registers
   * (x0 = the segment's first non-NaN value) and writes final bins, or, where
   * the row range is split without group alignment, per-chunk triples that
   * the combine folds in chunk order with the same merge. Error 16 without
   * out_ssd, 6 without another member's buffer. No finish mode applies
   * (error 14). */
  FH_SET_SUMMARY = 14,
  /* single-pass arg-reductions, COLUMN path only (fh_grouped_reduce returns
   * error 18 without launching): each thread keeps, per column, the running
   * extremum of the segment, its row, the first NaN row and the non-NaN
   * count in registers, so the values are read once. Outputs, (ngroups, m):
   * out_sum = int64 original row perm[i] + row_offset of the extremum
   * (INT64_MAX where no candidate was seen), out_count = non-NaN rows,
   * out_present = any row seen, out_nanflag = a NaN row seen. Ties go to the
   * smallest row (np.argmin / np.argmax) under ANY perm that sorts the
   * codes: equal values compare rows. Equality is that of the values
   * (-0.0 == +0.0), not of an encoding. Without FH_SKIPNAN the smallest NaN
   * row of a group wins and stays the winner; with it NaN rows are no
   * candidates, do not count, and still set out_nanflag. Where the row range
   * is split without group alignment, each chunk writes (value, row, NaN
   * row) and the combine merges them by the same rules. `target` is refused
   * (error 19). */
  FH_SET_ARGMIN_COLS = 15,
  FH_SET_ARGMAX_COLS = 16,
};

/* flags */
enum fh_flags {
  FH_SKIPNAN = 1 << 0,    /* nan* reductions: NaN values contribute nothing */
  FH_FORCE_LDS = 1 << 1,  /* testing: force the LDS-binned path */
  FH_FORCE_ATOMIC = 1 << 2, /* testing: force the global-atomic path */
  FH_SORTED_LABELS = 1 << 3, /* caller guarantees labels are nondecreasing and
                              * all in [0, ngroups): fh_grouped_scan skips the
                              * radix sort (the reference's issorted fast path,
                              * aggregate_flox.py:9-23) */
  FH_NO_HOST_SYNC = 1 << 4, /* stream is being captured into a hipGraph: only
                             * paths with no D2H readback / stream sync may
                             * run (LDS, sorted-direct, atomic — NOT the
                             * bucket-partition paths, whose overflow check
                             * and counting pre-pass synchronize) */
};

/* finish modes: the LDS-binned path's combine kernel can write the finished
 * aggregation (one value per group, in `result`) instead of the partials.
 * Each mode belongs to one op set; masked groups receive `fill`:
 * masked = has_fill && (min_count > 0 ? count < min_count : group empty),
 * "empty" being present == 0 where the set has a present flag, else
 * count == 0. Any call that cannot be served this way returns error 14. */
enum fh_finish {
  FH_FINISH_NONE = 0,
  FH_FINISH_MEAN = 1,  /* FH_SET_SUM_COUNT: (double)sum / (double)count */
  FH_FINISH_SUM = 2,   /* FH_SET_SUM_COUNT_PRESENT: the sum */
  FH_FINISH_COUNT = 3, /* FH_SET_COUNT: the count */
};

typedef struct fh_call {
  int op_set;     /* fh_opset */
  int vdtype;     /* fh_dtype of `values` */
  int ldtype;     /* fh_ldtype of `labels` (and `labels2`) */
  int flags;      /* fh_flags */
  int64_t n;      /* rows */
  int64_t ngroups;
  /* 2-D groupby (reference factorize.py:102-108 _ravel_factorized):
   * labels2 != NULL means code = labels[i]*g1 + labels2[i], with either
   * label out of [0,g0)/[0,g1) meaning "not in any group" (the reference's
   * -1 sentinel). ngroups must equal g0*g1. */
  const void* values;
  const void* labels;
  const void* labels2;
  int64_t g0, g1;
  /* per-group means (f64[ngroups]) for FH_SET_SSD, else NULL */
  const double* means;

  /* outputs: each f64/i64/u32[ngroups]; only the set's members are written.
   * out_sum: f64 for float inputs (also receives the SSD result), i64 for
   *          int inputs. out_min/out_max: in VALUE dtype, +inf/-inf
   *          (INT_MAX/MIN) for empty groups. */
  void* out_sum;
  int64_t* out_count;
  uint32_t* out_present;
  void* out_min;
  void* out_max;
  uint32_t* out_nanflag;

  /* scratch: device buffer of fh_scratch_bytes() bytes (may be NULL when 0) */
  void* scratch;
  int64_t scratch_bytes;

  void* stream;   /* hipStream_t */
  int path_used;  /* out: 1 = LDS-binned, 2 = global-atomic, 3 = column */

  /* column path only (fh_grouped_reduce_cols): array is (n rows x m
   * columns), element (t,c) at values[t*ldm + c]; labels then holds the
   * int32 group codes SORTED ascending and perm the int32 argsort
   * permutation; outputs are (ngroups, m) group-major. */
  const void* perm;
  int64_t m, ldm;
  /* optional: group-aligned row chunking (int64[nchunks+1] row offsets, each
   * chunk covering disjoint groups -> chunks write final bins directly, no
   * slab); when NULL the launcher row-splits with a partials slab instead */
  const void* chunk_offsets;
  int64_t nchunks;
  /* FH_SET_IDXMIN/IDXMAX: per-group match targets (value dtype, nullable)
   * and the global row offset of this shard (multi-GPU arg-reductions) */
  const void* target;
  int64_t row_offset;
  /* optional (nullable): uint16[n], 16-byte aligned. When set on an
   * int64/int32-label call that takes the LDS-binned path, the pass also
   * writes each row's final code (labels[i], or labels[i]*g1 + labels2[i]
   * for 2-D; 0xFFFF for a row in no group) — the FH_L_U16 input of later
   * calls over the same labels. Error 13 on any other path. */
  void* emit_codes;
  /* finish mode (fh_finish; 0 = write partials as above). When set, none of
   * the out_* buffers is touched: `result` ([ngroups] of result_dtype, an
   * fh_dtype: FH_F32/FH_F64 for mean, those or FH_I64 for sum/count)
   * receives the value converted with a plain C cast, or `fill` cast the
   * same way where the group is masked. */
  int finish;
  int result_dtype;
  void* result;
  int64_t min_count;
  int has_fill;
  double fill;
  /* FH_SET_SUMMARY: f64[ngroups] sum of squared deviations about the mean */
  void* out_ssd;
} fh_call;

/* scratch requirement for this call (0 when the global-atomic path is used,
 * and for an FH_SET_SUMMARY call that would be refused: off the LDS-binned
 * path in 1-D, without out_ssd on the column path) */
int64_t fh_scratch_bytes(const fh_call* c);

/* which path fh_grouped_reduce would take for this call, without running
 * it: 1 = LDS-binned, 0 = anything else (partition / sorted-direct /
 * global-atomic), < 0 on a malformed call. Only op_set, vdtype, ngroups and
 * flags are read. */
int fh_query_path(const fh_call* c);

/* run the fused grouped reduction; returns 0 on success */
int fh_grouped_reduce(fh_call* c);

/* grouped reduce over the leading/strided axis of a multi-column array
 * (the reference's axis-subset case, core.py:272-316 + factorize.py:24-39,
 * computed without offsetting labels: one segmented pass per column) */
int fh_grouped_reduce_cols(fh_call* c);

/* 1 where fh_grouped_reduce_cols serves the op set, 0 where it does not (an
 * unknown set included). Libraries older than the column forms of
 * FH_SET_IDXMIN/IDXMAX and FH_SET_ARG*_COLS lack the symbol. */
int fh_cols_supports(int op_set);

/* grouped quantiles / mode over the leading axis of a multi-column array:
 * the column form of fh_grouped_quantile. Inputs as fh_grouped_reduce_cols
 * (values n x m with row stride ldm, labels = int32 codes in [-1, ngroups)
 * sorted ascending, perm = the int32 sorting permutation, any perm that sorts
 * the codes); `means` carries the device q array (f64[nq]) as it does for
 * fh_grouped_quantile; FH_SKIPNAN in flags. max_seg_rows is the caller's
 * upper bound on any group's row count: one workgroup stages one group's
 * rows for a tile of columns in LDS, sorts them there and answers every q
 * (include/floxhip_qcols.h has the tile plan), so the values are read once,
 * in place, with no scratch, no host sync and no limit on n * m. A group
 * longer than max_seg_rows gets an unspecified result (memory-safe).
 * Outputs: nq > 0: out_sum = f64 [nq][ngroups][m]; nq == 0 (mode): out_sum =
 * value dtype [ngroups][m]; out_count (nullable) = int64 [ngroups][m] non-NaN
 * rows of each (group, column). Results equal fh_grouped_quantile's bit for
 * bit (the same selection rules run on the sorted keys); mode treats -0.0 as
 * +0.0. path_used = 3. Errors (no launch, outputs untouched): 20 =
 * max_seg_rows beyond fh_quantile_cols_max_rows(vdtype); 21 = a missing
 * buffer (values, labels, perm, out_sum, or means with nq > 0) or a negative
 * / out-of-int32 extent; 9 = unknown value dtype. fh_error_string predates
 * codes 20 and 21. Came without a new revision (fh_call is unchanged): a
 * caller detects it by the symbol. */
int fh_grouped_quantile_cols(fh_call* c, int nq, int64_t max_seg_rows);
/* the longest segment fh_grouped_quantile_cols can stage for this value
 * dtype (2048 for all four); 0 for an unknown dtype */
int64_t fh_quantile_cols_max_rows(int vdtype);

/* the same quantiles for groups of any length, by radix selection: inputs,
 * FH_SKIPNAN, `means` = device q (f64[nq]), out_sum = f64 [nq][ngroups][m]
 * and the nullable out_count as fh_grouped_quantile_cols takes them, without
 * max_seg_rows. One workgroup serves one group's rows for a tile of columns:
 * it refines the order-preserving key of every wanted rank one 8-bit digit
 * per read of the segment, most significant first, in per-column LDS
 * histograms (include/floxhip_selcols.h has the tile plan), so there is no
 * capacity, no scratch, no host sync and no limit on n * m; more q than one
 * launch has slots for are served in batches. Results equal
 * fh_grouped_quantile's and fh_grouped_quantile_cols' bit for bit (the same
 * interpolation rule runs on the selected keys). nq >= 1: the mode is not
 * served. path_used = 3. Errors (no launch, outputs untouched): 22 = a
 * missing buffer (values, labels, perm, out_sum, means), nq < 1, or a
 * negative / out-of-int32 extent (within this entry; fh_grouped_scan_cols
 * gives the number its own meaning); 9 = unknown value dtype. Came without a
 * new revision (fh_call is unchanged): a caller detects it by the symbol. */
int fh_grouped_quantile_select_cols(fh_call* c, int nq);

/* grouped scans over the leading axis of a multi-column array: the column
 * form of fh_grouped_scan, op as there (0 cumsum, 1 nancumsum, 2 ffill,
 * 3 bfill). Inputs as fh_grouped_reduce_cols: values n x m with row stride
 * ldm and unit column stride, labels = int32 codes in [-1, ngroups) sorted
 * ascending, perm = the int32 permutation of a STABLE sort of the codes. A
 * scan depends on the row order inside a group, so, unlike the arg sets,
 * "any perm that sorts the codes" is NOT enough: equal codes must keep their
 * original row order. chunk_offsets / nchunks (optional) are group-aligned
 * row chunks as there: one workgroup walks (column tile, chunk), and a chunk
 * must be a whole number of runs of equal codes; nchunks <= 65535. Without
 * them one workgroup per column tile walks all rows. Every run of equal codes
 * is a segment and scans as one group, the -1 run included (the reference's
 * NaN-sentinel group). out_sum receives value-dtype n x m with row stride
 * ldo: element (perm[i], c) goes to out_sum[perm[i] * ldo + c]; out_sum must
 * not overlap values. cumsum adds sequentially in the value dtype in row
 * order, the segment's first row initialising the sum (-0.0 survives, a NaN
 * poisons the rest of its segment, int64 wraps); nancumsum the same with NaN
 * contributing 0; ffill carries the last non-NaN value and leaves NaN before
 * the first; bfill is ffill walked from the segment's last row. Served:
 * sums for FH_F32 / FH_F64 / FH_I64, fills for FH_F32 / FH_F64. The values
 * are read once and written once, in place, with no scratch, no host sync and
 * no limit on n * m (offsets are 64-bit; n itself fits int32). ngroups is
 * not read. path_used = 3. Errors (no launch, outputs untouched): 22 = a
 * missing buffer (values, labels, perm, out_sum); 23 = a negative extent, n
 * beyond int32, a row stride below m, or nchunks out of range; 24 = an
 * unknown op or a (dtype, op) pair that is not served. fh_error_string
 * predates these codes. Came without a new revision (fh_call is unchanged): a
 * caller detects it by the symbol. */
int fh_grouped_scan_cols(fh_call* c, int op, int64_t ldo);

/* the row form of the same scans, for the other layout: values m lead rows x
 * n time steps with the grouped (time) axis the contiguous one, element
 * (r, t) at values[r * ldm + t], ldm >= n. labels = int32 codes, n of them,
 * in the caller's ORIGINAL time order, each in [-1, ngroups): no sort and no
 * perm. ngroups is read: a row's running value of every group but the current
 * one waits in LDS, (ngroups + 1) values per row, which bounds the group count
 * (include/floxhip_scanrows.h has the tile plan; fh_scan_rows_max_groups
 * answers for a dtype). out_sum receives value-dtype m x n with row stride
 * ldo and must not overlap values. Per lead row the semantics are exactly
 * fh_grouped_scan_cols': every distinct code is a group, the -1 steps one of
 * them; sequential adds in the value dtype in time order, so results equal
 * the column form's bit for bit on the same data. Served: sums for FH_F32 /
 * FH_F64 / FH_I64, fills for FH_F32 / FH_F64. The values are read once and
 * written once, in place: no scratch, no D2H copy, no stream synchronize and
 * no chunk plan, so the entry can run on a stream under hipGraph capture; no
 * limit on n * m (offsets are 64-bit; n itself fits int32). path_used = 3.
 * Errors (no launch, outputs untouched), numbered as fh_grouped_scan_cols
 * numbers them: 22 = a missing buffer (values, labels, out_sum); 23 = a
 * negative extent, n beyond int32, or a row stride below n; 24 = an unknown
 * op or a (dtype, op) pair that is not served; 25 = ngroups beyond
 * fh_scan_rows_max_groups for the dtype. Came without a new revision (fh_call
 * is unchanged): a caller detects it by the symbol. */
int fh_grouped_scan_rows(fh_call* c, int op, int64_t ldo);
/* the largest ngroups fh_grouped_scan_rows serves for a value dtype; 0 for a
 * dtype it does not serve */
int64_t fh_scan_rows_max_groups(int vdtype);
/* the tile of that call: lead rows per workgroup and time steps per tile.
 * Returns 0, or the code fh_grouped_scan_rows would refuse with (23 negative
 * ngroups, 24 dtype, 25 capacity), the outputs untouched. */
int fh_scan_rows_plan(int vdtype, int64_t ngroups, int* row_tile, int* time_tile);

/* pack (order-preserving 32-bit value encoding, global row index) into one
 * int64 key per row, so that a grouped MIN over the keys is argmin/argmax
 * with np.argmin's first-occurrence tie-break (the packed form of the
 * reference's argreduce, flox/aggregate_flox.py:151-187). FH_F32/FH_I32
 * values only; requires n + row_offset < 2^32. out: int64[n]. */
int fh_pack_argkeys(const void* values, int vdtype, int64_t n,
                    int64_t row_offset, int ismax, int skipnan, void* out,
                    void* stream);

/* packed label codes (include/floxhip_codes.h): bytes of the packed buffer
 * for n rows at width 12 or 14 (whole 1024-row tiles; -1 for another
 * width), and the pass that rewrites uint16[n] codes (the emit_codes output)
 * into it: 0xFFFF becomes the all-ones W-bit code, as do the padding slots
 * of the last tile. out: 16-byte aligned. Every code below 0xFFFF must be
 * below 2^W - 1, which holds when the emitting call had ngroups <= 2^W - 2. */
int64_t fh_packed_code_bytes(int64_t n, int width);
int fh_pack_codes(const void* u16, int64_t n, int width, void* out,
                  void* stream);

const char* fh_error_string(int code);
int fh_version(void);
/* append-only revisions of fh_call within one fh_version: 2 added
 * emit_codes, FH_L_U16 and fh_query_path; 3 added the finish fields; 4 added
 * FH_SET_SUMMARY and out_ssd; 5 added FH_L_P12/FH_L_P14, fh_pack_codes and
 * fh_packed_code_bytes; 6 added FH_SET_SUMMARY to fh_grouped_reduce_cols. A
 * caller built against revision R
 * needs a library with fh_abi_revision() >= R. The column forms of
 * FH_SET_IDXMIN/IDXMAX, FH_SET_ARGMIN_COLS/ARGMAX_COLS and fh_cols_supports
 * came without a new revision (it stays 6: fh_call is unchanged): a caller
 * detects them by the fh_cols_supports symbol and its answer. Likewise
 * fh_grouped_quantile_cols, fh_grouped_scan_cols,
 * fh_grouped_quantile_select_cols and fh_grouped_scan_rows, each by its own
 * symbol. */
int fh_abi_revision(void);

#ifdef __cplusplus
}
#endif
#endif /* FLOXHIP_H */
