// One byte per pixel of a packed sample, written as aligned 32-bit words: what instances.hip (the instance map) and follow.hip (the
// followed masks) both do.  A sample's pixels are walked from the aligned word its first byte lies in: with a = (address of the sample's
// first byte) & 3, pixel p sits at position p + a of that walk, a wave takes 64 consecutive positions starting at a multiple of 4, and
// the four bytes of an aligned word sit in four neighbouring lanes.
#pragma once
#include "common.h"

namespace udet {

// Lane `lane` of a wave holds the byte v of pixel p of a sample of HW pixels whose bytes start at mp (valid: 0 <= p < HW; v of an invalid
// lane is not stored).  Every lane of the wave calls this.  The first lane of a word stores it when all four of its pixels are the
// sample's; the at most three head and tail bytes the sample shares a word with its neighbours go one by one.
__device__ __forceinline__ void store_packed_byte(unsigned char* __restrict__ mp, long long p, long long HW, int lane, bool valid, unsigned v) {
  const unsigned word = v | ((unsigned)__shfl_down((int)v, 1) << 8) | ((unsigned)__shfl_down((int)v, 2) << 16) |
                        ((unsigned)__shfl_down((int)v, 3) << 24);
  const long long p0 = p - (lane & 3);
  if (p0 >= 0 && p0 + 3 < HW) {
    if ((lane & 3) == 0) *reinterpret_cast<unsigned*>(mp + p0) = word;
  } else if (valid) {
    mp[p] = (unsigned char)v;  // the sample's head and tail
  }
}

}  // namespace udet
