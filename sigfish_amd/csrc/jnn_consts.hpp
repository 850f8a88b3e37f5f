// jnn_consts.hpp -- the constants of the adaptor and poly-A segmenters (src/jnn.c, src/jnn.h) behind the RNA automatic query start,
// shared by the batch kernels (events_kernels.hpp) and the session's (events_auto_stream.hpp) so that the two cannot drift apart.
#pragma once

namespace sfa {

constexpr int kAdWindow = 2000, kAdSegDist = 1500, kAdHi = 200000;                  // jnnv2() with JNNV2_RNA_*_ADAPTOR
constexpr int kPaCorrector = 50, kPaSegDist = 200, kPaWindow = 250, kPaError = 30;  // jnn_core() with JNNV1_*_POLYA

}  // namespace sfa
