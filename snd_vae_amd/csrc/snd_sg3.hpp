#pragma once
#include "snd_common.hpp"

namespace snd {
// Parameter offsets (floats) of one SpatialGraphConvolution_3D layer; the layout of
// include/snd_vae.h (snd_sg3_param_count).
struct Sg3POff { long long M0, b0, M1, b1, M2, b2, M3, b3, gamma, beta, total; };
Sg3POff sg3_poff(int F, int h0, int h1, int h2, int h3);
}  // namespace snd
