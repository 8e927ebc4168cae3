// mt_jump.h -- jump-ahead polynomials of the MT19937 word stream (host side, mt_jump.hip).
#pragma once
#include <stdint.h>

#include <vector>

namespace skr {

constexpr int MT_JUMP_DEG = 19937;   // degree of the characteristic polynomial phi of the one-word transition
constexpr int MT_JUMP_WORDS = 624;   // uint32 words of a polynomial of degree < MT_JUMP_DEG (bit i = coefficient of x^i)

// out[k] = x^(e0 + k * step) mod phi for k < count (MT_JUMP_WORDS words each), cached for the life of the process by
// exponent: a size class seen before costs a map lookup.  The first call finds phi (Berlekamp-Massey, tens of ms).
// Returns false if phi could not be found (it always can for MT19937).  Thread-safe.
bool mt_jump_polys(int64_t e0, int64_t step, int count, std::vector<const uint32_t*>& out);

}  // namespace skr
