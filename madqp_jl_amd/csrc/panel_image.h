// The packed image of a factored panel of width w, as it travels between chol.hip (which writes it) and the grid path
// (dist.hip / dist_core.inc, which broadcasts, files and reads it):
//   [info, 0 | inverse 128-blocks of the panel, ceil(w/128) images [Wcm | Wrm] | L, w columns]
// Plain C++: the CPU build of the grid schedule (tests/csrc/dist_cpu.cpp) includes it too.
#pragma once
#include <cstdint>

constexpr int64_t IMG_NB = 128;                     // order of an inverse block
constexpr int64_t IMG_HDR = 2;                      // doubles: [info, 0] (keeps the payload 16-byte aligned)
constexpr int64_t IMG_WBLK = 2 * IMG_NB * IMG_NB;   // doubles per inverse block image [Wcm | Wrm]
inline int64_t img_nblk(int64_t w) { return (w + IMG_NB - 1) / IMG_NB; }
inline int64_t img_blocks(int64_t w) { return img_nblk(w) * IMG_WBLK; }    // doubles of the inverse blocks
inline int64_t img_L(int64_t w) { return IMG_HDR + img_blocks(w); }        // offset of L
inline int64_t img_count(int64_t w, int64_t rows) { return img_L(w) + rows * w; }  // whole image, L of `rows` rows
