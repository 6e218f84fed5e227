// lane_rows.inc -- the device skeleton of the lane-per-record filters (DESIGN 4n; the host half is filter_host.hpp): the table's
// way into LDS, the row loop every wave walks in step, the counting of a wave's rows and the grid's size.  What a row is, what is
// counted and where it goes stays with each filter.  Included inside namespace flbgpu after kdev.inc.

// the most blocks a launch gets: 65536, or what the test switch FLBGPU_LANE_MAX_BLOCKS names (filter_host.cpp)
unsigned lane_max_blocks();

// one block per BLOCK rows up to the cap; the row loops stride over the rest
template <uint32_t BLOCK> static unsigned lane_blocks(uint64_t n) {
    const uint64_t blocks = (n + BLOCK - 1) / BLOCK, cap = lane_max_blocks();
    return (unsigned) (blocks > cap ? cap : blocks);
}

// the table's words into the front of g_lds.  No barrier: the caller issues the one __syncthreads() behind everything it stages.
template <uint32_t BLOCK> DEV LDS_AS uint32_t *lane_stage_table(const uint32_t *table, uint32_t bytes) {
    LDS_AS uint32_t *lds = (LDS_AS uint32_t *) g_lds;
    for (uint32_t i = threadIdx.x; i < bytes / 4; i += BLOCK) lds[i] = table[i];
    return lds;
}

// f(r, live) for the rows of this lane, a wave's 64 rows a trip.  Every wave walks in step (the trip count is the wave's, not the
// lane's): every lane enters f on every trip, live or not, so the ballots and shuffles inside f see whole waves.
template <uint32_t BLOCK, class F> DEV void lane_wave_rows(uint64_t n, F f) {
    const uint64_t gsz = (uint64_t) gridDim.x * BLOCK;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r0 = (uint64_t) blockIdx.x * BLOCK + (threadIdx.x & ~63u); r0 < n; r0 += gsz) f(r0 + lane, r0 + lane < n);
}

DEV unsigned long long lane_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a call-level fact of a wave's 64 rows: counted by lane 0 from the ballot (the whole wave is here).  Returns the ballot.
DEV unsigned long long lane_count(unsigned long long &counter, bool fact) {
    const unsigned long long b = __ballot(fact);
    if ((threadIdx.x & 63u) == 0) counter += __popcll(b);
    return b;
}

// one atomic per counter that is not zero
DEV void lane_flush(unsigned long long *counter, unsigned long long n) { if (n) atomicAdd(counter, n); }
