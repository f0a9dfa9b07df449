// javarandom.hpp -- java.util.Random as the JDK documents it (48-bit LCG).  The reference seeds
// k-means++ with (Random. 42) (src/hnsw/ann/partition/ivf_flat.clj:36) and draws HNSW levels from
// (Random.) (src/hnsw/ultra_fast.clj:139-147), and the LSH hyperplanes from (Random. 42)'s nextGaussian
// (src/hnsw/ann/hash/hybrid_lsh.clj:24-31,80); using the same generator keeps a JVM user's seeds
// meaningful on this engine.
#pragma once
#include <stdint.h>

#include <cmath>

namespace hg {

class JavaRandom {
   public:
    explicit JavaRandom(int64_t seed) : seed_((static_cast<uint64_t>(seed) ^ 0x5DEECE66DULL) & kMask) {}
    int32_t next(int bits) {
        seed_ = (seed_ * 0x5DEECE66DULL + 0xBULL) & kMask;
        return static_cast<int32_t>(static_cast<int64_t>(seed_ >> (48 - bits)));
    }
    int32_t next_int(int32_t bound) {
        int32_t r = next(31);
        int32_t m = bound - 1;
        if ((bound & m) == 0) return static_cast<int32_t>((static_cast<int64_t>(bound) * r) >> 31);
        for (int32_t u = r;
             static_cast<int32_t>(static_cast<uint32_t>(u) - static_cast<uint32_t>(r = u % bound) +
                                  static_cast<uint32_t>(m)) < 0;
             u = next(31)) {
        }
        return r;
    }
    double next_double() {
        int64_t hi = next(26), lo = next(27);
        return static_cast<double>((hi << 27) + lo) * 0x1.0p-53;
    }
    // nextGaussian as the JDK documents it: the polar method, two values per accepted point, the second one cached.  (The JDK
    // takes StrictMath.log / sqrt; this is libm's -- sqrt is correctly rounded in both, the last bit of log may differ.)
    double next_gaussian() {
        if (have_gaussian_) {
            have_gaussian_ = false;
            return gaussian_;
        }
        double v1, v2, s;
        do {
            v1 = 2 * next_double() - 1;
            v2 = 2 * next_double() - 1;
            s = v1 * v1 + v2 * v2;
        } while (s >= 1 || s == 0);
        const double mul = std::sqrt(-2 * std::log(s) / s);
        gaussian_ = v2 * mul;
        have_gaussian_ = true;
        return v1 * mul;
    }

   private:
    static constexpr uint64_t kMask = (1ULL << 48) - 1;
    uint64_t seed_;
    double gaussian_ = 0.0;
    bool have_gaussian_ = false;
};

}  // namespace hg
