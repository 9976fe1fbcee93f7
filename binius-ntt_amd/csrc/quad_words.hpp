// LDS slot sizes of the lane-group products (quad_mul.hpp) and the sumcheck's degree bound. No HIP
// header: the device code (quad_mul.hpp) and the host-only round planner (sc_rounds.hpp) share them.
#pragma once

namespace bn {
namespace quad {

constexpr int kRowWords = 36;    // LDS words per 32-word row (padding: bank spread)
constexpr int kQuadWords = 304;  // LDS words per quad slot (8 padded rows + spread)
constexpr int kMaxD = 8;
constexpr int kHexWords = 24 * kRowWords + 16;  // hex_mul: 24 rows
constexpr int kWideZ16 = 24 * kRowWords;        // wide_mul: hex_mul's rows, then the GF(2^16) products
constexpr int kWideWords = kWideZ16 + 36 * 20 + 16;

}  // namespace quad
}  // namespace bn
