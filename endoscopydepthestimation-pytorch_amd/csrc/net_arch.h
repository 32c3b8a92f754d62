// FC-DenseNet57 (reference models.py:100-187) as the two host schedules see it (net.hip: fp32, net16.hip: 16-bit storage): its widths, and
// ONE walk of its modules in .parameters() order, which lays out the flat parameter tensor and the BatchNorm tables both families index.
// Plain C++, no HIP: a host compiler builds it alone.  Nothing here knows how either family lays out its level buffers.
#pragma once

#include <stdint.h>

#include <vector>

namespace endo {

constexpr int kLevels = 5;                // resolutions of the down / up path; level kLevels is the bottleneck
constexpr int kLayers = 4;                // dense layers per block
constexpr int kGrowth = 12;               // maps a dense layer adds
constexpr int kFirst = 48;
constexpr int kNew = kGrowth * kLayers;   // 48: maps a dense block adds
constexpr float kBnEps = 1.0e-5f;
constexpr float kBnMomentum = 0.1f;

constexpr int down_in(int level) { return kFirst + kNew * level; }          // C_L: input of down block L (and, L = kLevels, of the bottleneck)
constexpr int up_in(int level) { return kNew + down_in(level) + kNew; }     // input of the up block at level L: transition-up output + skip
constexpr int kBottIn = down_in(kLevels);                                   // 288
constexpr int kFinalIn = up_in(0) + kNew;                                   // 192

// down[i][j] and td[i] at level i; bottleneck[j]; tu[i] and up[i][j] in the order the up path runs them, at level kLevels - 1 - i
enum class Role { First, Down, Td, Bott, Tu, Up, Final };
inline bool is_dense(Role r) { return r == Role::Down || r == Role::Bott || r == Role::Up; }

// g, b (gamma, beta; weight, bias): offsets in floats of the flat parameter tensor.  c: width; index: among the BatchNorms, module order; run: the
// running mean in the flat running-statistics tensor (the running variance follows, c floats on); before: channels of all BatchNorms before it
struct BnDesc { int c; int64_t g, b; int index; int64_t run, before; };
// level: whose pixel grid the output is computed on (td: before the pooling); bn: index of the BatchNorm -> ReLU in front of it, -1: none
struct ConvDesc { Role role; int i, j, level; int cout, cin, ks; int64_t w, b; int bn; };
inline int dense_base(const ConvDesc& m) { return m.cin - kGrowth * m.j; }          // a dense layer's block input width

struct Arch {
    std::vector<ConvDesc> convs;                 // 56, module order
    std::vector<BnDesc> bns;                     // 49
    std::vector<int64_t> param_offsets;          // 210 tensors in .parameters() order
    int64_t param_floats = 0, bn_floats = 0, bn_width = 0;
};

inline const Arch& arch() {
    static const Arch* a = [] {
        Arch* a = new Arch();
        auto tensor = [&](int64_t floats) { const int64_t at = a->param_floats; a->param_offsets.push_back(at); a->param_floats += floats; return at; };
        auto conv = [&](Role role, int i, int j, int level, int cout, int cin, int ks, bool bn) {
            ConvDesc m{role, i, j, level, cout, cin, ks, 0, 0, -1};
            if (bn) {
                m.bn = static_cast<int>(a->bns.size());
                const int64_t g = tensor(cin), b = tensor(cin);
                a->bns.push_back({cin, g, b, m.bn, a->bn_floats, a->bn_width});
                a->bn_floats += 2 * cin; a->bn_width += cin;
            }
            m.w = tensor(static_cast<int64_t>(cout) * cin * ks * ks);
            m.b = tensor(cout);
            a->convs.push_back(m);
        };
        conv(Role::First, 0, 0, 0, kFirst, 3, 3, false);
        for (int l = 0; l < kLevels; ++l) for (int j = 0; j < kLayers; ++j) conv(Role::Down, l, j, l, kGrowth, down_in(l) + kGrowth * j, 3, true);
        for (int l = 0; l < kLevels; ++l) conv(Role::Td, l, 0, l, down_in(l) + kNew, down_in(l) + kNew, 1, true);
        for (int j = 0; j < kLayers; ++j) conv(Role::Bott, 0, j, kLevels, kGrowth, kBottIn + kGrowth * j, 3, true);
        for (int i = 0; i < kLevels; ++i) conv(Role::Tu, i, 0, kLevels - 1 - i, kNew, kNew, 3, false);
        for (int i = 0; i < kLevels; ++i) for (int j = 0; j < kLayers; ++j) conv(Role::Up, i, j, kLevels - 1 - i, kGrowth, up_in(kLevels - 1 - i) + kGrowth * j, 3, true);
        conv(Role::Final, 0, 0, 0, 1, kFinalIn, 1, false);
        return a;
    }();
    return *a;
}

// The modules as a family's schedule addresses them, each entry a copy of its description; Conv: ConvDesc plus what the family adds to it.
template <typename Conv>
struct ModuleTable {
    Conv first, final_;
    Conv down_conv[kLevels][kLayers], td_conv[kLevels], bott_conv[kLayers], tu_conv[kLevels], up_conv[kLevels][kLayers];
    BnDesc down_bn[kLevels][kLayers], td_bn[kLevels], bott_bn[kLayers], up_bn[kLevels][kLayers];
    // m's entry and (m.bn >= 0) its BatchNorm's, by Role in its order: i < kLevels and j < kLayers for every module, so each candidate is an element
    Conv& conv(const ConvDesc& m) {
        Conv* at[] = {&first, &down_conv[m.i][m.j], &td_conv[m.i], &bott_conv[m.j], &tu_conv[m.i], &up_conv[m.i][m.j], &final_};
        return *at[static_cast<int>(m.role)];
    }
    BnDesc& bn(const ConvDesc& m) {
        BnDesc* at[] = {nullptr, &down_bn[m.i][m.j], &td_bn[m.i], &bott_bn[m.j], nullptr, &up_bn[m.i][m.j], nullptr};
        return *at[static_cast<int>(m.role)];
    }
    ModuleTable() {
        for (const ConvDesc& m : arch().convs) {
            static_cast<ConvDesc&>(conv(m)) = m;
            if (m.bn >= 0) bn(m) = arch().bns[m.bn];
        }
    }
};

}  // namespace endo
