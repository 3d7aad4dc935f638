/* drs_device_weights.h -- per-sample weights (SparseLengthsWeightedSum, drs_weights.h) on the device-array path
 * (drs_device_inputs.h, drs_device_outputs.h): one entry point of libdrs_hip.so beyond the symbol set of drs.h, which
 * includes this file inside its extern "C" block; do not include it on its own.
 *
 * drs_stage_batch_weights attaches weights to a STAGED batch from host arrays.  A model with weighted bags whose features
 * live in HBM had to download the weights, stage a batch, attach them and serve by batch id.  Here the weights are one more
 * device array per query: the set's ONE input-pass launch (input_pass.hip) copies -- or widens -- them into the slot's own
 * fp32 weight block beside narrowing the indices, and the set is gathered exactly as staged weighted batches in the same
 * composition are: the same kernels, the same bits.  The symbol set of drs.h is unchanged and DRS_ABI_VERSION stays 5. */
#ifndef DRS_DEVICE_WEIGHTS_H_
#define DRS_DEVICE_WEIGHTS_H_

/* drs_run_queues_device_multi_async / drs_run_queues_device_io_multi_async with per-sample weights.  The first eleven
 * arguments mean exactly what they mean in drs_run_queues_device_multi_async; d_out, out_row_stride, stream and ordered
 * mean exactly what they mean in drs_run_queues_device_io_multi_async.  d_out == NULL is the HOST-output form (results
 * through drs_wait only): `ordered` must then be 0, and out_row_stride and stream are ignored.  Every refusal, every
 * device-found error, the NaN rule, the lifetime and the ordering rules of those two calls hold unchanged; the weight
 * arrays are inputs like the others -- read, never written; complete when the call is made (ordered == 0) or ordered
 * behind `stream` (ordered == 1); alive and untouched until drs_wait on the slot has returned.
 *
 * d_weights[i]: query i's weights, [T, n_idx_per_table[i]] -- one per index, laid out like d_ids[i] -- rows
 * wgt_row_stride[i] ELEMENTS apart, elements of wgt_dtype[i]: 0 fp32 | 1 fp16 | 2 bf16 (the DRS_TABLE_* codes; a NULL
 * wgt_dtype table means fp32 throughout).  The pointer is aligned to its element, no more: a column slice of a wider
 * tensor, an odd row stride work.  A NULL d_weights[i] means query i is unweighted (wgt_row_stride[i] and wgt_dtype[i] are
 * not read); a set may mix weighted and unweighted queries as sets of staged batches may, and an unweighted query keeps
 * its sequential bits there.  The three tables themselves are HOST arrays.
 *
 * Widening.   fp16 and bf16 weights are widened to fp32 exactly (torch's per_sample_weights have the table's dtype, so a
 *             half-precision model hands half weights); the bits are those of the upcast weights handed as fp32.
 * Summation.  The chain drs_stage_batch_weights states: acc = fma(w_j, row_j, acc) in index order under "sls_exact" 1, the
 *             same per-row step in the split order otherwise.  The launch form is the one the same set takes as staged
 *             weighted batches: the ring walk or the any-width form, the flat and one-lookup forms under
 *             "sls_weighted_flat" 1 (dispatch log: a "w" token).
 * Unweighted. A call whose d_weights entries are all NULL is the corresponding unweighted call: the same launches, the
 *             same bits, the same dispatch log.
 * Non-finite weights are outside the contract, as for staged batches: a weight is data and is never checked.  Where the
 * pass finds a bad INDEX the set is in error (drs_wait reports it, device outputs hold NaN) whatever its weights are.
 *
 * Refused before anything is enqueued (synchronously; nothing changes, the slot stays free), after the refusals of
 * drs_run_queues_device_multi_async and before those drs_run_queues_device_io_multi_async makes about its outputs:
 *   DRS_ERR_BAD_ARG      a NULL d_weights or wgt_row_stride table; ordered != 0 with d_out == NULL
 *   DRS_ERR_UNSUPPORTED  a non-NULL d_weights[i] on a DIN or DIEN handle (they pool by the plain sum only) or under
 *                        "sls_pool" 1 (there is no weighted mean)
 *   DRS_ERR_BAD_ARG      for a non-NULL d_weights[i]: wgt_dtype[i] outside {0, 1, 2}; a negative wgt_row_stride[i], or
 *                        one so large that the extent -- (T - 1) * stride + n_idx_per_table[i] elements -- would exceed
 *                        2^60 bytes; a pointer not aligned to its element; the pointer check of drs_device_inputs.h
 *                        (plain device memory of the engine's device whose extent ends inside its allocation), an empty
 *                        query's pointer included
 *   DRS_ERR_OOM          the slot's weight block -- DRS_MAX_COALESCE * T * max_batch * max_lookups floats, allocated when
 *                        the slot first sees a weighted set and kept until drs_destroy -- could not be allocated         */
int32_t drs_run_queues_device_weighted_multi_async(
    drs_handle h, int32_t slot, int32_t n, const int32_t* bs,
    const float* const* d_dense, const int64_t* const* d_ids, const int64_t* ids_row_stride,
    const int64_t* n_idx_per_table, const int32_t* const* d_lengths, const int64_t* len_row_stride,
    const int32_t* fixed_len /*[n] or NULL*/,
    const void* const* d_weights /*[n]; an entry may be NULL*/, const int64_t* wgt_row_stride /*[n], ELEMENTS*/,
    const int32_t* wgt_dtype /*[n] or NULL = all fp32; 0 fp32 | 1 fp16 | 2 bf16 (the DRS_TABLE_* codes)*/,
    float* const* d_out /*NULL: results through drs_wait only*/, const int64_t* out_row_stride,
    void* stream, int32_t ordered);

#endif /* DRS_DEVICE_WEIGHTS_H_ */
