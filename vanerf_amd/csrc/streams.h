// streams.h -- the one description of the streams a packed weight handle can carry.  The host packer (weights_pack.cpp), the pack and the
// download (api.cpp), the device packer (weights_update.hip) and the launches index this table; none of them knows a stream by name except
// the kernel launch that reads it.
#pragma once
#include "../../include/vanerf_hip.h"

namespace vanerf {

enum Stream { // the ABI's `which`
    STREAM_FP32 = VANERF_STREAM_FP32, STREAM_BF16X3 = VANERF_STREAM_BF16X3, STREAM_BACKWARD = VANERF_STREAM_BACKWARD,
    STREAM_HOISTED = VANERF_STREAM_HOISTED, STREAM_LEAN = VANERF_STREAM_LEAN, STREAM_LEAN_BIAS = VANERF_STREAM_LEAN_BIAS,
    STREAM_LEAN_FOLDED = VANERF_STREAM_LEAN_FOLDED,
    STREAM_NONE = 7,       // never a stream: the first `which` both calls refuse stays refused
    STREAM_TEXEL = 8,      // the texel level's bf16x3 stream (layer_spec.h, level 3): the lean stream with two layers cut to their scalar k-pairs
    STREAM_TEXEL_BIAS = 9, // a second copy of the bias table directly behind it (the kernel reads stream and table through one buffer)
    NUM_STREAMS
};
// How a stream comes out of the effective weights `eff` (weights_pack.cpp): a gather through its placement table, out[i] = id ? eff[id - 1] : 0,
// one id per float (GATHER_F32) or two per 32-bit word of two bf16 (GATHER_BF16X3: low half's id | part << 30, high half's id; part 0 = the
// high bf16 part of the value, 1 the low one), or the folded matrices' slice of eff itself (EFF_SLICE).
enum StreamKind { GATHER_F32, GATHER_BF16X3, EFF_SLICE };
// The device allocations of a handle.  BLOCK_MAIN holds the handle's BLOCK_MAIN streams back to back in this table's order: the kernels of a
// bf16x3 handle see [forward | hoisted | lean | bias table | texel | bias table].
enum StreamBlock { BLOCK_MAIN, BLOCK_BACKWARD, BLOCK_EFF, NUM_BLOCKS };
enum : unsigned { MODE_FP32 = 1u << 0, MODE_BF16X3 = 1u << 1 }; // bit `mode` of vanerf_weights_pack

struct StreamSpec { StreamKind kind; unsigned modes; StreamBlock block; };
constexpr StreamSpec kStreams[NUM_STREAMS] = {
    {GATHER_F32, MODE_FP32, BLOCK_MAIN},       // STREAM_FP32
    {GATHER_BF16X3, MODE_BF16X3, BLOCK_MAIN},  // STREAM_BF16X3
    {GATHER_F32, MODE_FP32, BLOCK_BACKWARD},   // STREAM_BACKWARD
    {GATHER_BF16X3, MODE_BF16X3, BLOCK_MAIN},  // STREAM_HOISTED
    {GATHER_BF16X3, MODE_BF16X3, BLOCK_MAIN},  // STREAM_LEAN
    {GATHER_F32, MODE_BF16X3, BLOCK_MAIN},     // STREAM_LEAN_BIAS: directly behind the lean stream, whose kernel reads both through one buffer
    {EFF_SLICE, MODE_BF16X3, BLOCK_EFF},       // STREAM_LEAN_FOLDED
    {GATHER_F32, 0u, BLOCK_MAIN},              // STREAM_NONE: no mode carries it, no placement
    {GATHER_BF16X3, MODE_BF16X3, BLOCK_MAIN},  // STREAM_TEXEL
    {GATHER_F32, MODE_BF16X3, BLOCK_MAIN},     // STREAM_TEXEL_BIAS: directly behind the texel stream
};
constexpr bool carries(int mode, int s) { return (kStreams[s].modes >> mode) & 1u; }
constexpr Stream forward_stream(int mode) { return mode ? STREAM_BF16X3 : STREAM_FP32; } // what the un-hoisted kernel of the mode runs on

} // namespace vanerf
