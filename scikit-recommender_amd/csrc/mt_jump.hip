// mt_jump.hip -- jump-ahead for the MT19937 word stream, host side (the device half: sampler.hip, 2e).
//
// The generator's state after word k is the 19937-bit window s_k = (top bit of x_k, x_{k+1} .. x_{k+623}) of the untempered
// words x; one word is a GF(2)-linear map T of it.  With phi the characteristic polynomial of T (phi(T) = 0) and
// x^e mod phi = sum_i c_i x^i, T^e = sum_i c_i T^i, and read word by word:
//     x_{e+j} = XOR over the set c_i of x_{i+j}            (1 <= j <= 624: every x_{i+j} there is a function of s_0)
// So the block array that starts at word e + 1 is a correlation of the words x_1 .. x_{19936+624} with the coefficients of
// one polynomial -- the low 31 bits of x_0, which s_0 does not hold, never enter.  Tempering is linear as well: the same sum
// holds for the tempered words the generator writes out.  phi comes from Berlekamp-Massey on the top bit of 2 * 19937 + 64
// words (the transition is primitive: any nonzero bit sequence of the generator has phi as its minimal polynomial).
#include "skr_common.h"
#include "mt_jump.h"

#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace {

constexpr int DEG = skr::MT_JUMP_DEG;
constexpr int W = (DEG + 63) / 64;     // 312 64-bit words: a polynomial of degree < DEG, and phi itself (degree DEG)
constexpr int MT_N = 624;
using Poly = std::vector<uint64_t>;

void mt_twist(uint32_t* mt) {          // the next block of std::mt19937, in place
    for (int k = 0; k < MT_N; ++k) {
        const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % MT_N] & 0x7fffffffu);
        mt[k] = mt[(k + 397) % MT_N] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
}

inline bool bit(const uint64_t* p, int64_t i) { return (p[i >> 6] >> (i & 63)) & 1u; }

// dst ^= src << sh, both n words long (what falls beyond n is dropped)
void xor_shifted(uint64_t* dst, const uint64_t* src, int n, int64_t sh) {
    const int64_t ws = sh >> 6;
    const int bs = static_cast<int>(sh & 63);
    for (int64_t w = n - 1 - ws; w >= 0; --w) {
        dst[w + ws] ^= src[w] << bs;
        if (bs && w + ws + 1 < n) dst[w + ws + 1] ^= src[w] >> (64 - bs);
    }
}

// Berlekamp-Massey over GF(2): the shortest C(x) = 1 + c_1 x + .. + c_L x^L with s_n = c_1 s_{n-1} + .. + c_L s_{n-L};
// phi(x) = x^L C(1/x)
bool find_phi(Poly& phi) {
    const int N = 2 * DEG + 64;
    const int NW = (N + 63) / 64 + 2;
    std::vector<uint32_t> mt(MT_N);
    mt[0] = 5489u;
    for (int i = 1; i < MT_N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + static_cast<uint32_t>(i);
    std::vector<uint64_t> rs(NW, 0);   // the bit sequence reversed (bit N-1-n = s_n): a sum over c_i s_{n-i} is a dot product
    for (int n = 0, k = MT_N; n < N; ++n, ++k) {
        if (k == MT_N) {
            mt_twist(mt.data());
            k = 0;
        }
        if (mt[k] >> 31) {
            const int r = N - 1 - n;
            rs[r >> 6] |= 1ull << (r & 63);
        }
    }
    std::vector<uint64_t> C(NW, 0), B(NW, 0), T(NW);
    C[0] = B[0] = 1;
    int L = 0, m = 1;
    for (int n = 0; n < N; ++n) {
        const int off = N - 1 - n, wo = off >> 6, bo = off & 63;
        uint64_t acc = 0;
        for (int w = 0; w <= (L >> 6); ++w) {
            uint64_t x = rs[wo + w] >> bo;
            if (bo) x |= rs[wo + w + 1] << (64 - bo);
            acc ^= C[w] & x;
        }
        if (!__builtin_parityll(acc)) {
            ++m;
            continue;
        }
        if (2 * L <= n) {
            T = C;
            xor_shifted(C.data(), B.data(), NW, m);
            L = n + 1 - L;
            B.swap(T);
            m = 1;
        } else {
            xor_shifted(C.data(), B.data(), NW, m);
            ++m;
        }
    }
    if (L != DEG) return false;
    phi.assign(W, 0);
    for (int k = 0; k <= L; ++k)
        if (bit(C.data(), L - k)) phi[k >> 6] |= 1ull << (k & 63);
    return true;
}

struct Jump {
    std::mutex mu;
    bool tried = false, ok = false;
    Poly phi;
    std::vector<uint64_t> phi_sh;             // phi << s for s < 64, W + 1 words each
    std::unordered_map<int64_t, Poly> pow;    // x^e mod phi by e (references stay valid while the map grows)
};

Jump& jump() {
    static Jump j;
    return j;
}

void shifted_copies(const uint64_t* a, std::vector<uint64_t>& out) {
    out.assign(64 * (W + 1), 0);
    for (int s = 0; s < 64; ++s)
        for (int w = 0; w <= W; ++w)
            out[s * (W + 1) + w] = (w < W ? a[w] << s : 0) | ((s && w > 0) ? a[w - 1] >> (64 - s) : 0);
}

// r = prod mod phi; prod holds 2 W + 1 words of a polynomial of degree <= 2 DEG - 2 and is destroyed
void reduce(const Jump& J, uint64_t* prod, uint64_t* r) {
    for (int64_t i = 2 * DEG - 2; i >= DEG; --i) {
        if (!bit(prod, i)) continue;
        const int64_t t = i - DEG;                 // prod ^= phi << t clears bit i and touches only bits below it
        const uint64_t* src = &J.phi_sh[(t & 63) * (W + 1)];
        uint64_t* dst = prod + (t >> 6);
        for (int k = 0; k <= W; ++k) dst[k] ^= src[k];
    }
    std::memcpy(r, prod, W * sizeof(uint64_t));
}

void mulmod(const Jump& J, const uint64_t* a, const uint64_t* b, uint64_t* r) {
    std::vector<uint64_t> ash, prod(2 * W + 1, 0);
    shifted_copies(a, ash);
    for (int w = 0; w < W; ++w)
        for (uint64_t m = b[w]; m; m &= m - 1) {
            const uint64_t* src = &ash[__builtin_ctzll(m) * (W + 1)];
            uint64_t* dst = &prod[w];
            for (int k = 0; k <= W; ++k) dst[k] ^= src[k];
        }
    reduce(J, prod.data(), r);
}

inline uint64_t spread32(uint32_t v) {     // bit i -> bit 2i
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

void sqrmod(const Jump& J, const uint64_t* a, uint64_t* r) {   // over GF(2): (sum a_i x^i)^2 = sum a_i x^2i
    std::vector<uint64_t> prod(2 * W + 1, 0);
    for (int w = 0; w < W; ++w) {
        prod[2 * w] = spread32(static_cast<uint32_t>(a[w]));
        prod[2 * w + 1] = spread32(static_cast<uint32_t>(a[w] >> 32));
    }
    reduce(J, prod.data(), r);
}

Poly xpow(const Jump& J, int64_t e) {      // x^e mod phi: square and shift from the top bit of e
    int b = 63 - __builtin_clzll(static_cast<uint64_t>(e) | 1u);
    int64_t pre = 0;                       // the leading bits of e while x^pre needs no reduction
    while (b >= 0 && ((pre << 1) | ((e >> b) & 1)) < DEG) {
        pre = (pre << 1) | ((e >> b) & 1);
        --b;
    }
    Poly r(W, 0), t(W);
    r[pre >> 6] = 1ull << (pre & 63);
    for (; b >= 0; --b) {
        sqrmod(J, r.data(), t.data());
        r.swap(t);
        if ((e >> b) & 1) {                // r *= x
            uint64_t carry = 0;
            for (int w = 0; w < W; ++w) {
                const uint64_t nc = r[w] >> 63;
                r[w] = (r[w] << 1) | carry;
                carry = nc;
            }
            if (bit(r.data(), DEG))
                for (int w = 0; w < W; ++w) r[w] ^= J.phi[w];
        }
    }
    return r;
}

}  // namespace

namespace skr {

bool mt_jump_polys(int64_t e0, int64_t step, int count, std::vector<const uint32_t*>& out) {
    Jump& J = jump();
    std::lock_guard<std::mutex> lock(J.mu);
    if (!J.tried) {
        J.tried = true;
        J.ok = find_phi(J.phi);
        if (J.ok) shifted_copies(J.phi.data(), J.phi_sh);
    }
    if (!J.ok) return false;
    out.resize(count);
    const Poly* prev = nullptr;
    const Poly* xs = nullptr;
    for (int k = 0; k < count; ++k) {
        const int64_t e = e0 + k * step;
        auto it = J.pow.find(e);
        if (it == J.pow.end()) {
            Poly p(W);
            if (prev) {                    // one product per polynomial after the first
                if (!xs) {
                    auto is = J.pow.find(step);
                    if (is == J.pow.end()) is = J.pow.emplace(step, xpow(J, step)).first;
                    xs = &is->second;
                }
                mulmod(J, prev->data(), xs->data(), p.data());
            } else {
                p = xpow(J, e);
            }
            it = J.pow.emplace(e, std::move(p)).first;
        }
        prev = &it->second;
        out[k] = reinterpret_cast<const uint32_t*>(prev->data());   // little-endian: bit i of word i / 32
    }
    return true;
}

}  // namespace skr

extern "C" int skr_mt_jump_host(const uint32_t* words624, int pos, int64_t n, uint32_t* out624, int* out_pos) {
    SKR_REQUIRE(words624 && out624 && out_pos, "skr_mt_jump_host: NULL argument");
    SKR_REQUIRE(pos >= 0 && pos <= MT_N, "skr_mt_jump_host: pos %d outside [0, 624]", pos);
    SKR_REQUIRE(n >= 0, "skr_mt_jump_host: negative n");
    const int64_t t = pos + n;             // the next word, counted from the first word of words624
    if (t <= MT_N) {
        std::memmove(out624, words624, MT_N * sizeof(uint32_t));
        *out_pos = static_cast<int>(t);
        return SKR_OK;
    }
    const int64_t b = t / MT_N * MT_N;     // first word of the block that holds it
    std::vector<const uint32_t*> pv;
    if (!skr::mt_jump_polys(b - 1, 0, 1, pv)) return skr::fail(SKR_EHIP, "MT19937: characteristic polynomial not found");
    const int nb = (DEG + 2 * MT_N - 1) / MT_N + 1;     // blocks x_0 .. holding x_{DEG - 1 + MT_N}
    std::vector<uint32_t> x(static_cast<size_t>(nb) * MT_N);
    std::memcpy(x.data(), words624, MT_N * sizeof(uint32_t));
    for (int k = 1; k < nb; ++k) {
        std::memcpy(&x[k * MT_N], &x[(k - 1) * MT_N], MT_N * sizeof(uint32_t));
        mt_twist(&x[k * MT_N]);
    }
    std::vector<uint32_t> acc(MT_N, 0);
    const uint32_t* c = pv[0];
    for (int i = 0; i < DEG; ++i)
        if ((c[i >> 5] >> (i & 31)) & 1u)
            for (int j = 0; j < MT_N; ++j) acc[j] ^= x[1 + i + j];
    std::memcpy(out624, acc.data(), MT_N * sizeof(uint32_t));
    *out_pos = static_cast<int>(t - b);
    return SKR_OK;
}
