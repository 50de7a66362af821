// What the device ingest (ingest_dev.hip) needs from the host ingest (csr.hip): the allocation rules of the CSR arrays, the
// stage timers of mispec_last_ingest_info, and the host path itself for the patterns whose structures are built from host arrays.
#pragma once
#include "csr.hpp"

namespace mispec {

// colind / val (codes) of A with the padding every SpMV kernel relies on, zero-filled on the context's stream; sets A.nnz.
// Throws Error(MISPEC_EINVAL) when nnz does not leave room for int32 row pointers.
void csr_alloc_entries(mispec_csr& A, int64_t nnz);
void csr_alloc_codes(mispec_csr& A);
// the calling thread's ten stage timers (seconds), see mispec_last_ingest_info
double* ingest_seconds();
// mispec_csr_upload's body on host arrays of the whole matrix, without resetting the timers: validation, formats, far statistic,
// reordering, staged image, tiles.  structurally_symmetric: the arrays come from a mirrored triangle.
mispec_csr* csr_upload_host(mispec_ctx* ctx, int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* colind,
                            const double* val, bool structurally_symmetric);

}  // namespace mispec
