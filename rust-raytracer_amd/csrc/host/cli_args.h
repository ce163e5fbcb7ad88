// cli_args.h — the command line of `raytracer <config_file> <output_file> [flags]` (main.cpp): every flag's value, and which flags may
// stand together.  No HIP, no globals, no I/O: parse() is a function of argv alone (tests/cliargs/cli_args_main.cpp runs it over
// tests/golden/cli_accept.json, every decision the driver has ever made).  The one check that needs the loaded scene (--passes greater
// than the scene's samples per pixel) is run()'s.
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

namespace cli {
// usage: the reference's usage line and a normal return (main.rs:9-12).  The other six are decided by --adaptive, --passes, --frames
// and --denoise, in this order of precedence (mode_of).
enum Mode { USAGE, ONE_SHOT, PROGRESSIVE, DENOISED_ONE_SHOT, ADAPTIVE, ANIMATION, DENOISED_ANIMATION };

struct Options {
  Mode mode = USAGE;
  const char* program = "";      // argv[0], for the usage line
  const char* config = nullptr;  // argv[1]
  const char* output = nullptr;  // argv[2]: the PNG, or with --frames the prefix of <prefix>_%03d.png
  int frames = 0;                // --frames N (0: none)
  bool frames_given = false;     // (--frames 0 is no animation, but it is an argument)
  double orbit = 0.0;            // --orbit DEG
  bool orbit_given = false;
  double shutter = -1.0;         // --shutter S in [0, 1]; < 0: not given
  long passes = 0;               // --passes K >= 1; 0: not given
  bool adaptive = false;         // --adaptive E
  double threshold = 0.0;        //   its E >= 0
  long min_spp = 16;             // --min-spp M in [1, 2^32)
  bool min_spp_given = false;
  bool denoise = false;          // --denoise
  bool flat_bvh = false;         // --flat-bvh
  std::string flat_frames;       // --flat-frames PREFIX; empty: not given
  long flat_rebuild = 0;         // --flat-rebuild K >= 1: every K-th frame's update rebuilds the structure, on the device; 0: not given
  bool t_surface = false;        // --temporal-surface
  double t_alpha = -1.0;         // --temporal-alpha A in [0, 1]; < 0: not given
  double t_alpha_specular = -1.0;  // --temporal-alpha-specular B in [0, 1]; < 0: not given
  double orbit_deg() const { return orbit_given ? orbit : 360.0 / frames; }  // the turn per frame: a full turn over the animation by default
};

inline Mode mode_of(const Options& o) {
  if (o.adaptive) return ADAPTIVE;
  if (o.passes > 0) return PROGRESSIVE;
  if (o.frames > 0) return o.denoise ? DENOISED_ANIMATION : ANIMATION;
  return o.denoise ? DENOISED_ONE_SHOT : ONE_SHOT;
}

// Which flag may appear in which mode, and which other flag it needs.  A flag outside its modes, or without the flag it needs: the usage line.
constexpr unsigned in(Mode a, Mode b = USAGE, Mode c = USAGE) { return (1u << a) | (1u << b) | (1u << c); }  // (USAGE: a bit no parsed mode has)
inline bool allowed(const Options& o, Mode mode) {
  const struct { bool given; unsigned modes; bool has_what_it_needs; } rules[] = {
      {o.frames != 0, in(ANIMATION, DENOISED_ANIMATION), true},  // (a count below zero makes no animation either: refused everywhere)
      {o.orbit_given, in(ANIMATION, DENOISED_ANIMATION), true},
      {o.shutter >= 0.0, in(ANIMATION, DENOISED_ANIMATION), true},
      {o.passes > 0, in(PROGRESSIVE), true},                     // (with --adaptive the mode is adaptive: refused)
      {o.min_spp_given, in(ADAPTIVE), true},                     // = needs --adaptive
      {o.denoise, in(PROGRESSIVE, DENOISED_ONE_SHOT, DENOISED_ANIMATION), true},
      {!o.flat_frames.empty(), in(ANIMATION), true},             // (moved flat primitives are not followed by the temporal filter)
      {o.flat_rebuild > 0, in(ANIMATION), !o.flat_frames.empty()},  // = needs --flat-frames (and a structure scene: run()'s check)
      {o.t_surface, in(DENOISED_ANIMATION), true},
      {o.t_alpha >= 0.0, in(DENOISED_ANIMATION), true},
      {o.t_alpha_specular >= 0.0, in(DENOISED_ANIMATION), o.t_surface},
      {mode == DENOISED_ANIMATION, ~0u, o.orbit_given},          // (a denoised animation names its turn per frame; 0 keeps the camera still)
      {o.frames_given, ~in(ONE_SHOT), true},                     // (`--frames 0` beside a mode is ignored; alone it is an argument of no mode)
  };  // (--adaptive E makes its mode and --flat-bvh goes with every mode: no row)
  for (const auto& r : rules)
    if (r.given && !((r.modes & (1u << mode)) && r.has_what_it_needs)) return false;
  return true;
}

// a whole number / a finite-or-not double that is all of s
inline bool whole(const char* s, long& v) { char* end = nullptr; v = std::strtol(s, &end, 10); return end != s && *end == '\0'; }
inline bool real(const char* s, double& v) { char* end = nullptr; v = std::strtod(s, &end); return end != s && *end == '\0'; }
inline bool unit_interval(const char* s, double& v) { return real(s, v) && v >= 0.0 && v <= 1.0; }

// The last occurrence of a flag wins, but --flat-bvh, --flat-frames or --flat-rebuild given twice is refused.  A flag without its value, an unknown flag, a
// malformed or out-of-range value: mode USAGE.  (--frames goes through atoi and --orbit through atof: `--frames x` is `--frames 0`.)
inline Options parse(int argc, char** argv) {
  Options o;
  if (argc > 0) o.program = argv[0];
  if (argc < 3) return o;
  o.config = argv[1];
  o.output = argv[2];
  bool ok = true;
  for (int i = 3; i < argc && ok; ++i) {
    const char* a = argv[i];
    auto is = [a](const char* name) { return !std::strcmp(a, name); };
    if (is("--denoise")) { o.denoise = true; continue; }
    if (is("--temporal-surface")) { o.t_surface = true; continue; }
    if (is("--flat-bvh")) { ok = !o.flat_bvh; o.flat_bvh = true; continue; }
    if (++i == argc) return o;  // (every other flag takes a value)
    const char* v = argv[i];
    if (is("--frames")) { o.frames = std::atoi(v); o.frames_given = true; }
    else if (is("--orbit")) { o.orbit = std::atof(v); o.orbit_given = true; }
    else if (is("--flat-frames")) { ok = o.flat_frames.empty() && v[0]; o.flat_frames = v; }
    else if (is("--flat-rebuild")) ok = o.flat_rebuild == 0 && whole(v, o.flat_rebuild) && o.flat_rebuild >= 1 && o.flat_rebuild <= 0x7FFFFFFFl;
    else if (is("--temporal-alpha")) ok = unit_interval(v, o.t_alpha);
    else if (is("--temporal-alpha-specular")) ok = unit_interval(v, o.t_alpha_specular);
    else if (is("--shutter")) ok = unit_interval(v, o.shutter);
    else if (is("--passes")) ok = whole(v, o.passes) && o.passes >= 1;
    else if (is("--adaptive")) { o.adaptive = true; ok = real(v, o.threshold) && o.threshold >= 0.0 && !std::isinf(o.threshold); }
    else if (is("--min-spp")) { o.min_spp_given = true; ok = whole(v, o.min_spp) && o.min_spp >= 1 && o.min_spp <= 0xFFFFFFFFl; }
    else ok = false;
  }
  if (ok && allowed(o, mode_of(o))) o.mode = mode_of(o);
  return o;
}
}  // namespace cli
