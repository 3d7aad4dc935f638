/* drs_device_inputs.h -- a launch set whose per-query arrays (dense rows, indices, bag lengths) are DEVICE arrays: two entry
 * points of libdrs_hip.so beyond the symbol set of drs.h, which includes this file inside its extern "C" block; do not
 * include it on its own.
 *
 * drs_run_queues_multi_async takes host arrays: it narrows the indices, builds the prefix sums of the lengths and runs
 * Caffe2's ENFORCEs on the CPU, and the result crosses the bus through a pinned block.  A caller whose features already
 * live in HBM (a PyTorch-ROCm pipeline) would copy them to the host for that.  Here ONE kernel launch per set does the
 * same pass on the device (input_pass.hip) and the set is then served exactly like a host set: the same kernels, the same
 * bits.  The symbol set of drs.h is unchanged and DRS_ABI_VERSION stays 5.                                             */
#ifndef DRS_DEVICE_INPUTS_H_
#define DRS_DEVICE_INPUTS_H_

/* drs_run_queues_multi_async with the three per-query arrays in device memory.  Query i is bs[i]; d_dense[i]: [bs, m_den]
 * fp32 (NULL where the model has no dense input); d_ids[i]: [T, n_idx_per_table[i]] int64, rows ids_row_stride[i]
 * ELEMENTS apart; d_lengths[i]: [T, bs] int32, rows len_row_stride[i] elements apart.  The pointer tables, strides and
 * counts themselves are HOST arrays.  n in 1..DRS_MAX_COALESCE; drs_wait returns the n results back to back; a query's
 * bits do not depend on what it was coalesced with, and they are the bits drs_run_queues_multi_async gives the same
 * arrays.  All six model kinds; per-sample weights travel on this path through drs_device_weights.h's form of this call
 * (the host per-call paths carry none).
 *
 * fixed_len[i] >= 0 is the caller's PROMISE that every bag of every table of query i holds exactly that many indices:
 * the host cannot look at the lengths, and the launch forms for fixed-length bags are chosen on the host.  fixed_len[i]
 * == -1, or fixed_len == NULL, means "read the lengths": the query is served by the ragged forms, as a host query with
 * unequal lengths is.  The promise is verified on the device (below).
 *
 * Ordering.   The arrays must be COMPLETE when the call is made: a caller that produced them on another stream
 *             synchronises it first (the rule of drs_sls / drs_fc / drs_interact_dot: the engine cannot order itself
 *             behind foreign work).
 * Lifetime.   The arrays must stay untouched and alive until drs_wait on that slot has returned.
 * Read-only.  The arrays are read, never written.
 *
 * Refused before anything is enqueued (synchronously; nothing changes, the slot stays free):
 *   DRS_ERR_BAD_ARG      a bad slot, n outside 1..DRS_MAX_COALESCE; a NULL table (fixed_len excepted); a NULL d_ids[i] or
 *                        d_lengths[i] with bs[i] > 0, a NULL d_dense[i] where the model has dense input and bs[i] > 0;
 *                        bs[i] outside [0, max_batch]; n_idx_per_table[i] negative or above the staging capacity
 *                        (max_batch * max_lookups); a negative row stride, or one so large that the extent below would
 *                        exceed 2^60 bytes; fixed_len[i] < -1; coalesced rows beyond the slot capacity (kept for
 *                        symmetry with the host form: the capacity is DRS_MAX_COALESCE * round_up(max_batch, 64)
 *                        rows, which n <= DRS_MAX_COALESCE queries of bs <= max_batch cannot exceed)
 *   DRS_ERR_LENGTHS_SUM  fixed_len[i] >= 0 and n_idx_per_table[i] != bs[i] * fixed_len[i]; bs[i] == 0 with indices
 *   DRS_ERR_BAD_ARG      the pointer check: every non-NULL data pointer (an empty query's too) must be plain device memory
 *                        (hipMemoryTypeDevice, not managed) of the engine's device, and its extent -- (T - 1) * stride +
 *                        count elements for ids and lengths, bs * m_den floats for dense -- must end inside its
 *                        allocation (hipMemGetAddressRange).  Pageable, pinned and managed host memory are all refused:
 *                        a mistaken pointer is an error string here, never a GPU page fault.
 *
 * Found on the device, reported by drs_wait (the call itself returned DRS_OK; no output is handed back; the next set on
 * the slot is served normally):
 *   DRS_ERR_LENGTHS_SUM  a negative length, sum(lengths[t]) != n_idx_per_table[i], or a length that differs from a
 *                        promised fixed_len (bit 2 of the slot's device error word)
 *   DRS_ERR_INDEX_RANGE  an index outside [0, rows_t), checked on the 64-bit value before it is narrowed (bit 0)
 *   When both are found, DRS_ERR_LENGTHS_SUM is reported.  Unlike the host path's message, this one names neither the
 *   position nor the value: the device keeps one word per slot.
 * Whatever the arrays hold, the launch set itself is safe: the pass stores row 0 in place of a bad index and clamps the
 * prefix sums into [0, n_idx], so a bad set costs one wasted launch set and an error code.                            */
int32_t drs_run_queues_device_multi_async(drs_handle h, int32_t slot, int32_t n, const int32_t* bs,
                                          const float* const* d_dense, const int64_t* const* d_ids,
                                          const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                          const int32_t* const* d_lengths, const int64_t* len_row_stride,
                                          const int32_t* fixed_len /*[n] or NULL*/);

/* the n == 1 form, scalar arguments (fixed_len: -1 = read the lengths) */
int32_t drs_run_queues_device_async(drs_handle h, int32_t slot, int32_t bs, const float* d_dense, const int64_t* d_ids,
                                    int64_t ids_row_stride, int64_t n_idx_per_table, const int32_t* d_lengths,
                                    int64_t len_row_stride, int32_t fixed_len);

#endif /* DRS_DEVICE_INPUTS_H_ */
