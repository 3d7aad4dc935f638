/* drs_device_outputs.h -- a launch set whose per-query arrays are DEVICE arrays (drs_device_inputs.h) and whose RESULTS stay on
 * the device too, ordered on a stream of the caller's if the caller wants: two entry points of libdrs_hip.so beyond the
 * symbol set of drs.h, which includes this file inside its extern "C" block; do not include it on its own.
 *
 * drs_run_queues_device_multi_async reads its inputs from HBM, but drs_wait still hands the scores back as host floats, and
 * the arrays must be complete when the call is made: a ranker that consumes the scores on the GPU uploads them again and
 * synchronises its stream once per set.  Here ONE more kernel launch per set (output_pass.hip) moves every query's scores
 * from the slot's device buffer to the caller's own device array, and two events tie the set to the caller's stream.  The
 * kernels that compute the scores, and their bits, are those of the host path.  The symbol set of drs.h is unchanged and
 * DRS_ABI_VERSION stays 5.                                                                                                */
#ifndef DRS_DEVICE_OUTPUTS_H_
#define DRS_DEVICE_OUTPUTS_H_

/* drs_run_queues_device_multi_async whose results go to device memory.  The first eleven arguments mean exactly what they
 * mean there; every refusal and every device-found error of that call holds unchanged.
 *
 * d_out[i], out_row_stride[i]: query i's scores go to d_out[i] as [bs[i], n_out] fp32, rows out_row_stride[i] FLOATS apart
 * (a column block of a wider score tensor works; the stride of a query of one row is not read).  d_out[i] may be NULL only
 * where bs[i] == 0.  The two tables themselves are HOST arrays.  The bits are the bits drs_wait hands the host.
 *
 * ordered == 0: today's contract at both ends.  `stream` is ignored; the inputs must be COMPLETE when the call is made;
 *               d_out is complete when drs_wait on the slot has returned.
 * ordered == 1: both ends ordered on `stream` (a hipStream_t; NULL is HIP's null stream and is valid -- PyTorch's default
 *               stream is that handle, which is why ordering is a flag of its own and not "non-NULL").
 * any other value: DRS_ERR_BAD_ARG.
 *
 * Ordering.   ordered == 1: the set is ordered behind everything already enqueued on `stream` -- the engine records an
 *             event of its own there and its input pass waits for it; the caller does not synchronise.  `stream` is then
 *             made to wait for the output pass: work the caller enqueues on `stream` AFTER the call has returned sees the
 *             finished d_out, with no host wait.  (The engine's streams are non-blocking: both edges are events, also
 *             for the null stream.)  A set of no samples (sum(bs) == 0) launches nothing and adds no edge.
 * Completion. drs_wait stays the slot's completion: drs_wait(h, slot, NULL, 0) returns the set's status, a non-NULL h_out
 *             still receives the host copy (the set still signs off on the host as every set does), and drs_wait returns
 *             only after the output pass has finished.  The next call on a busy slot waits for it first, as every entry
 *             point does.
 * Lifetime.   Inputs AND outputs must stay alive, and untouched by the caller, until drs_wait on that slot (or the next
 *             call on it) has returned -- also under ordered == 1: a caching allocator that recycles a tensor by ITS
 *             stream's order does not know the engine's streams.  Reading d_out on `stream` behind the call is the point
 *             and is fine.
 * Written.    Exactly the bs[i] * n_out floats of each query: nothing between the rows of a strided output, nothing of an
 *             empty query's array.  The input arrays are read, never written.
 * Overlap.    The byte extents -- (bs - 1) * stride + n_out floats -- of two queries' outputs must not overlap (refused,
 *             below: two column blocks of ONE wider tensor interleave and are refused too; give them to different sets
 *             or use row blocks).  d_out overlapping an INPUT array of the set is outside the contract and is NOT
 *             checked: it is the caller's responsibility.
 *
 * Refused before anything is enqueued (synchronously; nothing changes, the slot stays free), each DRS_ERR_BAD_ARG, after
 * the refusals of drs_run_queues_device_multi_async:
 *   ordered outside {0, 1}; a NULL d_out or out_row_stride table; a NULL d_out[i] with bs[i] > 0; a d_out[i] that is not
 *   4-byte aligned; out_row_stride[i] < n_out where bs[i] > 1 (negative strides among them); a stride so large that the
 *   extent would exceed 2^60 bytes; the pointer check of drs_device_inputs.h on every non-NULL d_out[i] (plain device
 *   memory of the engine's device, hipMemoryTypeDevice and not managed, whose extent ends inside its allocation:
 *   hipMemGetAddressRange); two queries' outputs that overlap.
 *
 * Found on the device (DRS_ERR_LENGTHS_SUM, DRS_ERR_INDEX_RANGE): reported by drs_wait exactly as for
 * drs_run_queues_device_multi_async.  A stream-ordered consumer may read d_out before anybody calls drs_wait, so the output
 * pass reads the slot's device error word itself:
 * NaN.        Where that word is non-zero, EVERY output element of EVERY query of the set receives the quiet NaN 0x7fc00000
 *             (the good queries of the set too: the device keeps one word per slot).  A consumer never sees plausible
 *             scores computed from clamped rows.                                                                          */
int32_t drs_run_queues_device_io_multi_async(drs_handle h, int32_t slot, int32_t n, const int32_t* bs,
                                             const float* const* d_dense, const int64_t* const* d_ids,
                                             const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                             const int32_t* const* d_lengths, const int64_t* len_row_stride,
                                             const int32_t* fixed_len /*[n] or NULL*/,
                                             float* const* d_out /*[n]*/, const int64_t* out_row_stride /*[n], floats*/,
                                             void* stream /*hipStream_t*/, int32_t ordered);

/* the n == 1 form, scalar arguments (fixed_len: -1 = read the lengths) */
int32_t drs_run_queues_device_io_async(drs_handle h, int32_t slot, int32_t bs, const float* d_dense, const int64_t* d_ids,
                                       int64_t ids_row_stride, int64_t n_idx_per_table, const int32_t* d_lengths,
                                       int64_t len_row_stride, int32_t fixed_len, float* d_out, int64_t out_row_stride,
                                       void* stream /*hipStream_t*/, int32_t ordered);

#endif /* DRS_DEVICE_OUTPUTS_H_ */
