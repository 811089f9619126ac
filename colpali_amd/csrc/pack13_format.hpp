// Sizes of one slab of the 13-bit corpus image; the layout is described in pack13.hip (the encoder) and read by maxsim_stream13.hip.
#pragma once

namespace msim {

constexpr int kSlab13Bytes = 6656;        // 32 rows x 128 values: 4096 low bytes + 2048 nibbles + 512 signs
constexpr int kSlab13Nib = 4096, kSlab13Sign = 6144;      // where the nibble and the sign planes start

}  // namespace msim
