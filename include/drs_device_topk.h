/* drs_device_topk.h -- each query's top-k rows from the GPU, one launch per launch set: two entry points of libdrs_hip.so
 * beyond the symbol set of drs.h, which includes this file inside its extern "C" block; do not include it on its own.
 *
 * A query is a user request with bs candidate items, scored in order to keep the best few.  drs_device_outputs.h leaves every
 * score of every sample on the device, and a ranker then launches one top-k per query -- up to 16 small launches per set,
 * and a row gather more where the rows carry several task scores.  Here ONE more kernel launch per set (topk_pass.hip) hands
 * back, for each query, the k samples that rank first by one score column: their row numbers and their full score rows.
 * The kernels that compute the scores, and their bits, are those of the host path.  The symbol set of drs.h is unchanged and
 * DRS_ABI_VERSION stays 5.
 *
 * Order.      The result is unique.  A score's bits map to a sortable 32-bit word: any NaN -> 0xffffffff (NaN ranks FIRST,
 *             as torch.topk has it), a negative value -> ~bits, everything else -> bits | 0x80000000; so +0.0 ranks above
 *             -0.0 and +inf below NaN.  Sample row r has the 64-bit key (word << 32) | (0xffffffff - r); the winners are the
 *             k LARGEST keys in descending order: equal scores rank by the LOWER row.  (deeprecsys_amd/csrc/topk_plan.h.) */
#ifndef DRS_DEVICE_TOPK_H_
#define DRS_DEVICE_TOPK_H_

#define DRS_TOPK_MAX 1024      /* the most rows one query hands back */

/* Operator level, beside drs_sls / drs_fc / drs_interact_dot: the top-k pass on an array of the caller's, as one query with
 * no error word, ENQUEUED on `stream` (a hipStream_t; NULL is HIP's null stream) -- the call returns at once and the
 * outputs are complete in stream order.
 *
 * d_scores: [rows, n_out] fp32, rows row_stride FLOATS apart (the stride of one row is not read); the rows rank by column
 * col.  d_idx receives the k winners' row numbers (int32, descending rank), d_top their rows as [k, n_out] contiguous fp32,
 * bit for bit.  Written: exactly those k int32 and k * n_out floats.  All three are plain device memory of the engine's
 * device; d_scores is read, never written, and must not overlap the outputs (not checked).
 *
 * Refused (DRS_ERR_BAD_ARG, nothing enqueued): rows < 1 or beyond 2^31 - 1; n_out < 1; k outside 1..min(rows, DRS_TOPK_MAX);
 * col outside [0, n_out); row_stride < n_out with more than one row, or an extent beyond 2^60 bytes; a NULL pointer, one not
 * 4-byte aligned, or one that fails the pointer check of drs_device_inputs.h (plain device memory of the engine's device
 * whose extent ends inside its allocation), on all three arrays; d_idx and d_top overlapping. */
int32_t drs_topk_rows(drs_handle h, const float* d_scores, int64_t rows, int32_t n_out, int64_t row_stride /*floats*/,
                      int32_t col, int32_t k, int32_t* d_idx /*[k]*/, float* d_top /*[k, n_out]*/, void* stream /*hipStream_t*/);

/* drs_run_queues_device_weighted_multi_async whose results are each query's top-k rows.  The first eleven arguments mean
 * exactly what they mean in drs_run_queues_device_multi_async; d_weights, wgt_row_stride and wgt_dtype exactly what they mean
 * in drs_device_weights.h, except that a NULL d_weights TABLE means the set is unweighted (the other two are then not
 * read); every refusal, every device-found error and every rule of those calls holds unchanged.  All six models: the pass
 * reads only the slot's score buffer, which every model's kernels fill.
 *
 * k[i]:       0..min(bs[i], DRS_TOPK_MAX).  At 0 nothing of query i is written and both its pointers may be NULL.
 * col:        the score column the rows rank by, 0 <= col < n_out (drs_out_width).
 * d_top_idx[i]:    int32 [k[i]] -- row numbers WITHIN query i, by descending rank (Order, above).
 * d_top_scores[i]: fp32 [k[i], n_out], contiguous -- the winners' full score rows, the bits drs_wait hands the host.
 * The k, d_top_idx and d_top_scores tables themselves are HOST arrays.
 *
 * stream, ordered: as in drs_run_queues_device_io_multi_async.
 * Ordering.   ordered == 1: the set is ordered behind everything already enqueued on `stream`, and `stream` is made to wait
 *             for the top-k pass: work enqueued there AFTER the call has returned sees the finished outputs, with no host
 *             wait.  ordered == 0: `stream` is ignored; the inputs must be complete when the call is made and the outputs
 *             are when drs_wait on the slot has returned.  The pass goes behind the set's last kernel; a set of no samples
 *             launches nothing and adds no edge.
 * Completion. drs_wait stays the slot's completion: it returns the set's status, a non-NULL h_out still receives EVERY
 *             score of the set (the set still signs off on the host as every set does), and it returns only after the
 *             top-k pass has finished.  The next call on a busy slot waits for it first.
 * Lifetime.   Inputs AND outputs must stay alive, and untouched by the caller, until drs_wait on that slot (or the next
 *             call on it) has returned -- also under ordered == 1.  Reading the outputs on `stream` behind the call is the
 *             point and is fine.
 * Written.    Exactly the k[i] int32 and k[i] * n_out floats of each query.
 * NaN.        Where the slot's device error word is non-zero (DRS_ERR_LENGTHS_SUM, DRS_ERR_INDEX_RANGE: reported by
 *             drs_wait), EVERY index written is -1 and EVERY score written is the quiet NaN 0x7fc00000, the good queries of
 *             the set too.  A consumer never sees plausible rows computed from clamped inputs.
 *
 * Refused before anything is enqueued (synchronously; nothing changes, the slot stays free), each DRS_ERR_BAD_ARG, after
 * the refusals of the device-input call and of drs_device_weights.h:
 *   ordered outside {0, 1}; col outside [0, n_out); a NULL k table; k[i] outside 0..min(bs[i], DRS_TOPK_MAX); a NULL
 *   d_top_idx or d_top_scores table where some k[i] > 0; a NULL or not 4-byte aligned d_top_idx[i] / d_top_scores[i] where
 *   k[i] > 0; the pointer check of drs_device_inputs.h on every such output (hipMemGetAddressRange); any two of the set's
 *   up to 32 outputs overlapping.  The outputs overlapping an INPUT array is outside the contract and is not checked.
 *
 * Dispatch log: one entry "topk_pass[<grid> x 256]" behind the set's, on this call only. */
int32_t drs_run_queues_device_topk_multi_async(
    drs_handle h, int32_t slot, int32_t n, const int32_t* bs,
    const float* const* d_dense, const int64_t* const* d_ids, const int64_t* ids_row_stride,
    const int64_t* n_idx_per_table, const int32_t* const* d_lengths, const int64_t* len_row_stride,
    const int32_t* fixed_len /*[n] or NULL*/,
    const void* const* d_weights /*[n] or NULL = unweighted; an entry may be NULL*/, const int64_t* wgt_row_stride /*[n], ELEMENTS*/,
    const int32_t* wgt_dtype /*[n] or NULL = all fp32*/,
    const int32_t* k /*[n]*/, int32_t col, int32_t* const* d_top_idx /*[n]*/, float* const* d_top_scores /*[n]*/,
    void* stream /*hipStream_t*/, int32_t ordered);

#endif /* DRS_DEVICE_TOPK_H_ */
