// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the digest a saved shard is verified by -- msim_digest over bytes in HBM and
// msim_digest_host, the same sum over host memory.  Host-side dispatch only: argument validation and launch on the caller's
// stream.  Nothing here allocates, frees or synchronises.  The kernel included below is defined and launched in this translation
// unit and in no other.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "digest.hip"

using namespace msim_abi;

static int digest_args(const char *who, const void *data, size_t nbytes, uint64_t pos, const void *acc) {
    if (!acc) return fail(MSIM_EINVAL, "%s: acc is NULL", who);
    if (!data && nbytes > 0) return fail(MSIM_EINVAL, "%s: data is NULL with nbytes=%zu", who, nbytes);
    if (pos % 8) return fail(MSIM_EINVAL, "%s: pos=%llu is not a multiple of 8", who, (unsigned long long)pos);
    if (misaligned(data, 8)) return fail(MSIM_EINVAL, "%s: data must be 8-byte aligned", who);
    return MSIM_OK;
}

extern "C" {

int msim_digest(const void *data, size_t nbytes, uint64_t pos, uint64_t *acc, void *stream) {
    if (int rc = digest_args("msim_digest", data, nbytes, pos, acc)) return rc;
    if (nbytes == 0) return MSIM_OK;
    const uint64_t n_full = (uint64_t)nbytes / 8;
    const int tail = (int)(nbytes % 8);
    const int head = (n_full > 0 && misaligned(data, 16)) ? 1 : 0;
    const uint64_t n_pairs = (n_full - (uint64_t)head) / 2;
    uint64_t blocks = (n_pairs + msim::kDigestBlock - 1) / msim::kDigestBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > (uint64_t)msim::kDigestMaxBlocks) blocks = msim::kDigestMaxBlocks;
    hipLaunchKernelGGL(msim::digest_kernel, dim3((unsigned)blocks), dim3(msim::kDigestBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint64_t *>(data), n_full, tail, head, pos / 8, reinterpret_cast<unsigned long long *>(acc));
    return launch_failed("digest_kernel");
}

int msim_digest_host(const void *data, size_t nbytes, uint64_t pos, uint64_t acc[2]) {
    if (int rc = digest_args("msim_digest_host", data, nbytes, pos, acc)) return rc;
    const uint64_t *words = static_cast<const uint64_t *>(data);
    const uint64_t n_full = (uint64_t)nbytes / 8, g0 = pos / 8;
    uint64_t a0 = 0, a1 = 0;
    for (uint64_t i = 0; i < n_full; ++i) msim::digest_word(words[i], g0 + i, a0, a1);
    if (nbytes % 8) {
        uint64_t w = 0;
        memcpy(&w, words + n_full, nbytes % 8);      // little-endian host: the bytes past the range stay zero
        msim::digest_word(w, g0 + n_full, a0, a1);
    }
    acc[0] += a0;
    acc[1] += a1;
    return MSIM_OK;
}

}  // extern "C"
