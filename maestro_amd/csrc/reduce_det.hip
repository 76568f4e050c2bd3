// Ordered fp32 column sums (mh_reduce_ordered, include/maestro_hip.h): the last hop of every reduction of the step in deterministic mode.
// One thread per destination column walks its chain of jobs in table order, every job in 16-row chunks; one plain store per
// column, no atomics, so the bits are a function of the operands and the table alone.
#include <algorithm>
#include <vector>

#include "reduce_det.hpp"

namespace {

__global__ __launch_bounds__(256) void reduce_ordered_kernel(const MhOrderedJob* __restrict__ jobs, int n_jobs,
                                                             const uint64_t* __restrict__ blocks) {
    const uint64_t e = blocks[blockIdx.x];
    const int j0 = (int)(e >> 32);
    if (j0 < 0 || j0 >= n_jobs) return;
    const MhOrderedJob first = jobs[j0];
    const long c = (long)(e & 0xFFFFFFFFu) * 256 + threadIdx.x;
    if (c >= first.cols) return;
    float acc = (first.flags & MH_ORDERED_ADD) ? first.dst[c] : 0.f;
    for (int j = j0; j < n_jobs; ++j) {          // the chain: the adjacent jobs with this destination
        const MhOrderedJob jb = jobs[j];
        if (jb.dst != first.dst) break;
        acc += ordered_job_total(jb.src + c, jb.rows, (size_t)jb.ld);
    }
    first.dst[c] = acc;
}

}  // namespace

extern "C" int mh_reduce_ordered(const MhOrderedJob* jobs_host, const MhOrderedJob* jobs_device, int n_jobs,
                                 const uint64_t* blocks_device, int n_blocks, void* stream) {
    MH_CHECK_ARG(jobs_host && jobs_device && blocks_device, "mh_reduce_ordered: null pointer (job tables, blocks)");
    MH_CHECK_ARG(n_jobs > 0 && n_blocks > 0, "mh_reduce_ordered: n_jobs %d and n_blocks %d must be positive", n_jobs, n_blocks);
    std::vector<const float*> closed;            // destinations of the chains that have ended
    for (int i = 0; i < n_jobs; ++i) {
        const MhOrderedJob& j = jobs_host[i];
        MH_CHECK_ARG(j.src && j.dst, "mh_reduce_ordered: job %d: null pointer", i);
        MH_CHECK_ARG(j.rows > 0 && j.cols > 0, "mh_reduce_ordered: job %d: rows %d, cols %d", i, j.rows, j.cols);
        MH_CHECK_ARG(j.cols <= j.ld, "mh_reduce_ordered: job %d: cols %d > ld %d", i, j.cols, j.ld);
        if (i > 0 && jobs_host[i - 1].dst == j.dst) {
            MH_CHECK_ARG(jobs_host[i - 1].cols == j.cols && jobs_host[i - 1].flags == j.flags,
                         "mh_reduce_ordered: job %d: cols / flags differ inside its chain", i);
        } else if (i > 0) {
            closed.push_back(jobs_host[i - 1].dst);
        }
    }
    std::sort(closed.begin(), closed.end());
    // a destination that was closed and appears again: two equal entries in `closed`, or the last chain's destination in it
    MH_CHECK_ARG(std::adjacent_find(closed.begin(), closed.end()) == closed.end() &&
                 !std::binary_search(closed.begin(), closed.end(), (const float*)jobs_host[n_jobs - 1].dst),
                 "mh_reduce_ordered: a chain is split apart in the table (jobs that share a dst must be adjacent)");
    hipLaunchKernelGGL(reduce_ordered_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, jobs_device, n_jobs, blocks_device);
    MH_LAUNCH_CHECK();
    return 0;
}
