// Shared by the two ConvUnit kernels in which one WAVE owns 32 consecutive frames of a clip end to end (conv_unit_fused.hip: fp32
// products; conv_unit_split.hip: bf16x3 products): the geometry of their common front end.  Lane (lj = lane & 31, lh = lane >> 5)
// computes dw_conv7 + LayerNorm of frame lj for the channels k = 8q + 4 lh + {0..3} it later feeds to the MFMAs as the B operand,
// from a per-wave LDS copy of the tile's 38 input rows.  Each kernel's geometry derives from this one and adds its weight buffers
// and its LDS carve.
//
// The front end's CODE is still written out in both kernels.  Moved into function templates here (parameter staging, row staging,
// the LayerNorm statistics, the residual store: each tried on its own) it compiles to other instructions than the text in place:
// hipcc simplifies a kernel and its helpers separately before it inlines them, and the operand order it settles on by then differs.
#pragma once

template <int C_, int XH_>  // XH: the input rows are staged in XH channel slices (LDS budget at C = 96)
struct Front32Geo {
    static constexpr int C = C_, XH = XH_;
    static constexpr int H4 = 4 * C;          // hidden width
    static constexpr int CT = (C + 31) / 32;  // output-channel tiles
    static constexpr int KQ = C / 8;          // k groups of 8 channels: a lane holds 4 of each
    static constexpr int XC = C / XH;         // channels per staged slice
    static constexpr int XS = XC + 4;         // padded row stride (odd number of 16-B slots: conflict-free b128)
    static constexpr int ROWS = 38;           // 32 frames + 3 + 3 halo
    static constexpr int xs_floats = ROWS * XS;
    static_assert(C % (8 * XH) == 0, "bad geometry");
};
