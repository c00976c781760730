// aipstack_amd -- linearising header-split Tx segments, the host side (plain C++, no HIP call):
// the argument checks of aipstack_tx_linearise / aipstack_tx_linearise_slotted and the copy
// pass's run length (the launchers are in linearise_kernels.hip).

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "linearise_common.h"

namespace aipstack_amd {

int tx_linearise_check_args(const void *d_hdr, uint64_t hdr_stride, const void *d_hdr_len,
                            const void *d_chunk_addr, const void *d_chunk_len,
                            const void *d_chunk_index, uint64_t n, const void *d_frames,
                            bool slotted, uint64_t slot_stride, const void *d_offsets,
                            uint32_t frame_max, const void *d_frame_len, const void *d_status) {
    if (!d_hdr || !d_hdr_len || !d_chunk_addr || !d_chunk_len || !d_chunk_index || !d_frames ||
        !d_frame_len || !d_status || (!slotted && !d_offsets))
        return AIPSTACK_CHKSUM_EINVAL;
    if (hdr_stride == 0 || frame_max == 0 || frame_max > AIPSTACK_CHKSUM_MAX_LEN ||
        n > kLinMaxSegments)
        return AIPSTACK_CHKSUM_EINVAL;
    if (slotted && (slot_stride == 0 || slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE ||
                    frame_max > slot_stride))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

uint32_t tx_linearise_run_frames(uint32_t frame_max) {
    const uint32_t r = 12288u / (frame_max ? frame_max : 1u);
    return r < 1u ? 1u : r > 64u ? 64u : r;
}

}  // namespace aipstack_amd
