// l2m_capi.cpp -- flbgpu_l2m_stale_dev / flbgpu_l2m_aggregate_dev (include/flb_gpu.h): log_to_metrics' stale scan and aggregation kernels
// (l2m_kernels.inc) on columns the caller supplies, for the tests (tests/test_l2m_edges_gpu.py).  The filters never call these; there is
// no other path behind them.
#include <stdint.h>
#include "host_int.hpp"

using namespace flbgpu;

static bool stale_dev(uint32_t *sid, uint64_t *val_bits, uint64_t n, uint64_t first_bad) {
    ScopedDevBuf d_sid, d_val, d_tmp, d_bad;
    const unsigned long long fb = first_bad;
    if (!d_sid.ensure((size_t) n * 4) || !d_val.ensure((size_t) n * 8) || !d_tmp.ensure(l2m_stale_tmp_elems(n) * 8) || !d_bad.ensure(8)) return false;
    HIPOK(hipMemcpy(d_sid.p, sid, (size_t) n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_val.p, val_bits, (size_t) n * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_bad.p, &fb, 8, hipMemcpyHostToDevice));
    launch_l2m_stale(d_sid.as<uint32_t>(), d_val.as<uint64_t>(), n, d_bad.as<unsigned long long>(), d_tmp.as<uint64_t>(), nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(nullptr));
    HIPOK(hipMemcpy(sid, d_sid.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(val_bits, d_val.p, (size_t) n * 8, hipMemcpyDeviceToHost));
    return true;
}

extern "C" int flbgpu_l2m_stale_dev(uint32_t *sid, uint64_t *val_bits, uint64_t n, uint64_t first_bad) {
    if (n == 0) return 0;
    if (!sid || !val_bits) { set_err("flbgpu_l2m_stale_dev: a column is missing"); return -1; }
    if (device_cus() <= 0) { set_err("flbgpu_init has not run: libflbgpu has no CPU path"); return -1; }
    return stale_dev(sid, val_bits, n, first_bad) ? 0 : -1;
}

static bool aggregate_dev(int mode, const uint32_t *sid, const uint64_t *val_bits, uint64_t n, uint64_t first_bad, uint64_t idx_base,
                          uint32_t nseries, int nb, const double *bounds, uint64_t *rows) {
    ScopedDevBuf d_sid, d_val, d_bad, d_rows, d_bounds, d_ns;
    const unsigned long long fb = first_bad;
    const int W = l2m_row_words(mode, nb);
    const size_t row_bytes = (size_t) nseries * W * 8;
    if (!d_sid.ensure((size_t) n * 4) || !d_val.ensure((size_t) n * 8) || !d_bad.ensure(8) || !d_rows.ensure(row_bytes) ||
        !d_bounds.ensure((size_t) (nb > 0 ? nb : 1) * sizeof(double)) || !d_ns.ensure(4)) return false;
    HIPOK(hipMemcpy(d_sid.p, sid, (size_t) n * 4, hipMemcpyHostToDevice));
    if (mode != L2M_COUNTER) HIPOK(hipMemcpy(d_val.p, val_bits, (size_t) n * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_bad.p, &fb, 8, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_rows.p, rows, row_bytes, hipMemcpyHostToDevice));
    if (nb > 0) HIPOK(hipMemcpy(d_bounds.p, bounds, (size_t) nb * sizeof(double), hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_ns.p, &nseries, 4, hipMemcpyHostToDevice));
    L2mAggArgs g;
    g.sid_col = d_sid.as<uint32_t>(); g.val_col = d_val.as<uint64_t>(); g.n = n;
    g.first_bad = d_bad.as<unsigned long long>();
    g.rows = d_rows.as<unsigned long long>(); g.W = W; g.mode = mode; g.nb = nb;
    g.bounds = d_bounds.as<double>(); g.idx_base = idx_base; g.n_series = d_ns.as<unsigned int>();
    launch_l2m_aggregate(g, device_cus(), nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(nullptr));
    HIPOK(hipMemcpy(rows, d_rows.p, row_bytes, hipMemcpyDeviceToHost));
    return true;
}

extern "C" int flbgpu_l2m_aggregate_dev(int mode, const uint32_t *sid, const uint64_t *val_bits, uint64_t n, uint64_t first_bad, uint64_t idx_base,
                                        uint32_t nseries, int nbuckets, const double *bounds, uint64_t *rows_inout) {
    if (mode != L2M_COUNTER && mode != L2M_GAUGE && mode != L2M_HISTOGRAM) { set_err("flbgpu_l2m_aggregate_dev: no such mode"); return -1; }
    if (mode != L2M_HISTOGRAM) nbuckets = 0;
    if (nbuckets < 0 || (nbuckets > 0 && !bounds)) { set_err("flbgpu_l2m_aggregate_dev: the bucket bounds are missing"); return -1; }
    if (n == 0 || nseries == 0) return 0;
    if (!sid || !rows_inout || (mode != L2M_COUNTER && !val_bits)) { set_err("flbgpu_l2m_aggregate_dev: a column is missing"); return -1; }
    if (device_cus() <= 0) { set_err("flbgpu_init has not run: libflbgpu has no CPU path"); return -1; }
    // the kernels trust the ids the extraction wrote: an id the row array has no room for is refused here
    const uint64_t lim = first_bad < n ? first_bad : n;
    for (uint64_t i = 0; i < lim; i++)
        if (sid[i] < L2M_SID_STALE && sid[i] >= nseries) { set_err("flbgpu_l2m_aggregate_dev: a series id is beyond nseries"); return -1; }
    return aggregate_dev(mode, sid, val_bits, n, first_bad, idx_base, nseries, nbuckets, bounds, rows_inout) ? 0 : -1;
}
