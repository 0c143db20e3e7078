// Process-wide configuration of the convolution family (conv_igemm.hip, conv_wgrad.hip, conv_pack.hip): the knobs behind
// fsraft_set_tuning / fsraft_get_tuning, the arithmetic switch of fsraft.h and the route record.  Host code only.
#include "conv_common.hpp"
#include <climits>

ConvKnobs knob;
__thread int t_route[2] = {0, 0};

namespace {
// every key of fsraft_tuning.h and the knob it sets (24 / 25 / 30 belonged to kernels that were removed)
const struct { int key; int ConvKnobs::*member; } KNOB_TABLE[] = {
    {FSRAFT_KEY_CONV_TILE, &ConvKnobs::conv_tile},
    {FSRAFT_KEY_WGRAD_TILE, &ConvKnobs::wgrad_tile},
    {FSRAFT_KEY_WGRAD_BLOCKS, &ConvKnobs::wgrad_blocks},
    {FSRAFT_KEY_CONV_ARITH, &ConvKnobs::conv_split},
    {FSRAFT_KEY_WGRAD_ARITH, &ConvKnobs::wgrad_split},
    {FSRAFT_KEY_CONV_BUF, &ConvKnobs::conv_buf},
    {FSRAFT_KEY_XCD_SWIZZLE, &ConvKnobs::xcd_swizzle},
    {FSRAFT_KEY_WGRAD_BUF, &ConvKnobs::wgrad_buf},
    {FSRAFT_KEY_CONV_N256, &ConvKnobs::conv_n256},
    {FSRAFT_KEY_WGRAD_MULTI, &ConvKnobs::wgrad_multi},
    {FSRAFT_KEY_WGRAD_BLOCKS_MULTI, &ConvKnobs::wgrad_blocks_multi},
    {FSRAFT_KEY_CONV_UNIFORM, &ConvKnobs::conv_uniform},
    {FSRAFT_KEY_CONV_W8, &ConvKnobs::conv_w8},
    {FSRAFT_KEY_CONV_W8_MIN, &ConvKnobs::conv_w8_min},
    {FSRAFT_KEY_WGRAD_W8, &ConvKnobs::wgrad_w8},
    {FSRAFT_KEY_WGRAD_PACK, &ConvKnobs::wgrad_pack},
    {FSRAFT_KEY_WGRAD_BLOCKS_PACK, &ConvKnobs::wgrad_blocks_pack},
    {FSRAFT_KEY_CONV_N64, &ConvKnobs::conv_n64},
    {FSRAFT_KEY_CONV_N64_MIN_M, &ConvKnobs::conv_n64_min_m},
    {FSRAFT_KEY_CONV_HALO, &ConvKnobs::conv_halo},
    {FSRAFT_KEY_CONV_HALO_MIN_M, &ConvKnobs::conv_halo_min_m},
    {FSRAFT_KEY_WGRAD_XCD, &ConvKnobs::wgrad_xcd},
    {FSRAFT_KEY_CONV_PATCH, &ConvKnobs::conv_patch},
    {FSRAFT_KEY_WGRAD_PATCH, &ConvKnobs::wgrad_patch},
    {FSRAFT_KEY_CONV_PATCH64, &ConvKnobs::conv_patch64},
    {FSRAFT_KEY_WGRAD_PATCH1, &ConvKnobs::wgrad_patch1},
    {FSRAFT_KEY_CONV_PATCH_MIN_M, &ConvKnobs::conv_patch_min_m},
    {FSRAFT_KEY_CONV_KSPLIT, &ConvKnobs::conv_ksplit},
};

int* knob_of(int key) {
  for (const auto& e : KNOB_TABLE)
    if (e.key == key) return &(knob.*e.member);
  return nullptr;
}
}  // namespace

extern "C" int fsraft_set_tuning(int key, int value) {
  int* k = knob_of(key);
  if (!k) return FS_ERR_ARG;
  *k = value;
  return FS_OK;
}

// Reads a knob back (INT_MIN: no such key).  The host side asks for the arithmetic-mode switches (key 3: forward /
// data-gradient convolutions, key 4: weight gradients) to skip packing the exact-fp32 weight matrices while the split-bf16
// kernels are the ones that run; the tests save and restore what they change.
extern "C" int fsraft_get_tuning(int key) {
  const int* k = knob_of(key);
  return k ? *k : INT_MIN;
}

extern "C" int fsraft_conv_last_route(int which) {
  return which == 0 || which == 1 ? t_route[which] : -1;
}

// fsraft.h: one switch for the arithmetic of every GEMM-shaped kernel of the library
extern "C" int fsraft_set_arithmetic(int mode) {
  if (mode != 0 && mode != 1) return FS_ERR_ARG;
  knob.conv_split = mode ? 1 : 0;
  knob.wgrad_split = mode ? 2 : 0;
  fsraft_set_build_split(mode);
  fsraft_set_gemm_split(mode);
  return FS_OK;
}
extern "C" int fsraft_get_arithmetic(void) { return knob.conv_split != 0 ? 1 : 0; }
