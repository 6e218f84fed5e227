// seqsum_capi.cpp -- flbgpu_seqsum_dev (include/flb_gpu.h): the reference-order sum's kernels (kernels_seqsum.hip) on columns the
// caller supplies, for the tests (tests/test_seqsum_gpu.py).  The filters never call this; there is no other path behind it.
#include <stdint.h>
#include "host_int.hpp"
#include "seqsum.hpp"

using namespace flbgpu;

static bool seqsum_dev(const uint32_t *sid, const uint64_t *val_bits, uint64_t n, uint32_t nseries, double *seq_inout) {
    ScopedDevBuf d_sid, d_val, d_seq, d_work;
    const size_t wb = seqsum_work_bytes(n, nseries);
    if (!d_sid.ensure((size_t) n * 4) || !d_val.ensure((size_t) n * 8) || !d_seq.ensure((size_t) nseries * sizeof(double)) || !d_work.ensure(wb)) return false;
    HIPOK(hipMemcpy(d_sid.p, sid, (size_t) n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_val.p, val_bits, (size_t) n * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_seq.p, seq_inout, (size_t) nseries * sizeof(double), hipMemcpyHostToDevice));
    if (!launch_seqsum_sorted(d_sid.as<uint32_t>(), d_val.as<uint64_t>(), n, d_seq.as<double>(), nseries, d_work.p, d_work.cap, nullptr)) {
        set_err("flbgpu_seqsum_dev: the reference-order sum failed to launch");
        return false;
    }
    HIPOK(hipStreamSynchronize(nullptr));
    HIPOK(hipMemcpy(seq_inout, d_seq.p, (size_t) nseries * sizeof(double), hipMemcpyDeviceToHost));
    return true;
}

extern "C" int flbgpu_seqsum_dev(const uint32_t *sid, const uint64_t *val_bits, uint64_t n, uint32_t nseries, double *seq_inout) {
    if (n == 0 || nseries == 0) return 0;
    if (!sid || !val_bits || !seq_inout) { set_err("flbgpu_seqsum_dev: a column is missing"); return -1; }
    return seqsum_dev(sid, val_bits, n, nseries, seq_inout) ? 0 : -1;
}
