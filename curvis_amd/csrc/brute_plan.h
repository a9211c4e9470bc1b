/* brute_plan.h -- what the brute renderer makes of one call, decided in ONE place: is the combination of options and call shape
 * refused (and in which words), which path renders it (fused or staged, relay or static), and which kernel family is launched.
 * Host only, plain C++17, no HIP and nothing of render_host.h: render_host.h builds the Facts, asks plan() and launches what it
 * names; tests/sanitize/san_brute_plan.cpp walks every combination of the facts.
 *
 * To read off what an option excludes, and under whose name the call is refused, look for its rows in kRefusals and for its
 * entry in kNoRelay.  A kernel family exists for the launch shapes family_exists() names and for no other: render_host.h
 * instantiates exactly those, and no plan that is not a refusal names a family that is absent for the call's shape. */
#pragma once

namespace brute {

constexpr int KIND_SCHWARZSCHILD = 3; /* CURVIS_METRIC_SCHWARZSCHILD (render_host.h asserts it) */
constexpr int STATIC_ONLY = 1;        /* Facts::variant of the seat belt's re-render: the static kernel, as option "variant" = 1 asks */
enum Disc { DISC_NONE, DISC_STATIC, DISC_MOVING };

/* everything the decision reads */
struct Facts {
  bool dump = false;          /* the debug dump is wanted */
  int variant = -1;           /* option "variant": -1 automatic, 0 persistent, 1 static, 2 relay; or STATIC_ONLY */
  bool fuse_shade = true;     /* options "fuse_shade", "fast_math" */
  bool fast_math = true;
  bool supersample = false;   /* option "supersample" > 1 */
  bool sky_filter = false;    /* options "sky_filter", "sky_mipmap" */
  bool sky_mipmap = false;
  bool projection = false;    /* option "projection" != 0 */
  bool step_scale = false;    /* option "step_scale" != 0 */
  bool integrator = false;    /* option "integrator" = 1 (Heun) */
  int disc = DISC_NONE;       /* a disc is set; DISC_MOVING: and its motion is not 0 */
  bool moving = false;        /* a frame of the call has a camera velocity */
  int kind = 0;               /* the metric's kind */
  bool relay_size_ok = false; /* the relay kernel's size conditions hold (render_host.h choose_render_path) */
};

/* ---- the kernel families and the launch shapes each exists for ------------------------------------------------------------ */
enum class Family {
  Persistent,  /* geodesic_persistent<KIND, PHI, FAST> */
  Unfused,     /* geodesic_static<KIND, PHI, FAST, false>: shade_kernel shades from the ray store */
  StagedAdapt, /* geodesic_static<KIND, true, FAST, false, 1, 0, 0, ADAPT>: the debug dump under scaled or Heun steps */
  Fused,       /* geodesic_static<KIND, false, FAST, true, SS, FILTER, PROJ, ADAPT> */
  Relay,       /* geodesic_relay<KIND, FAST, SS, FILTER, PROJ> */
  Disc,        /* geodesic_static<KIND, true, FAST, true, SS, FILTER, PROJ, ADAPT, 1> */
  DiscMotion   /* ... DISC = 2 */
};
/* the template arguments of a launch (render_host.h LaunchShape) as values.  ss stands for the factor: 1, or any of 2, 4, 8 */
struct Shape {
  int kind;
  bool fast;
  int ss, filter, proj, adapt;
};
constexpr bool family_exists(Family f, const Shape &s) {
  if (s.adapt != 0 && !s.fast) return false; /* no such shape: the ADAPT kernels exist for the fast step only */
  const bool plain = s.ss == 1 && s.filter == 0 && s.proj == 0; /* all a staged kernel holds: single rays, nearest lookup, perspective */
  const bool schwarzschild = s.kind == KIND_SCHWARZSCHILD;
  switch (f) {
    case Family::Persistent: return plain && s.adapt == 0 && !schwarzschild;
    case Family::Unfused: return plain && s.adapt == 0;
    case Family::StagedAdapt: return plain && s.adapt != 0;
    case Family::Fused: return true;
    case Family::Relay: return s.adapt == 0 && s.filter != 2 && !schwarzschild;
    case Family::Disc: return true;
    case Family::DiscMotion: return schwarzschild;
  }
  return false;
}
template <typename S> /* S: a LaunchShape */
constexpr bool family_exists(Family f) {
  return family_exists(f, Shape{S::KIND, S::FAST, S::SS, S::FILTER, S::PROJ, S::ADAPT});
}
/* the shape a call with these facts is launched in (with_launch_shape's arguments: prepare_call_shape makes FILTER = 2 of the
 * mip-mapped lookup, a moving camera travels as a projection bit, and the strict step has ADAPT = 0 only -- step_scale_kappa
 * refuses the options that would need more) */
constexpr Shape launch_shape(const Facts &f) {
  return Shape{f.kind, f.fast_math, f.supersample ? 2 : 1, f.sky_mipmap ? 2 : f.sky_filter ? 1 : 0, f.projection || f.moving ? 1 : 0,
               !f.fast_math ? 0 : f.integrator ? 2 : f.step_scale ? 1 : 0};
}

/* ---- the refusals, as data ------------------------------------------------------------------------------------------------- */
enum class Is { /* one fact about the call; a row of kRefusals refuses the call when both of its facts hold */
  Disc, DiscMotion, Moving, Mipmap, Projection, Filter, Supersample, StepScale, Integrator, Schwarzschild, NotSchwarzschild,
  Dump, Persistent /* variant = 0 */, Unfused /* fuse_shade = 0 */, UnfusedNoDump
};
constexpr bool holds(const Facts &f, Is w) {
  switch (w) {
    case Is::Disc: return f.disc != DISC_NONE;
    case Is::DiscMotion: return f.disc == DISC_MOVING;
    case Is::Moving: return f.moving;
    case Is::Mipmap: return f.sky_mipmap;
    case Is::Projection: return f.projection;
    case Is::Filter: return f.sky_filter;
    case Is::Supersample: return f.supersample;
    case Is::StepScale: return f.step_scale;
    case Is::Integrator: return f.integrator;
    case Is::Schwarzschild: return f.kind == KIND_SCHWARZSCHILD;
    case Is::NotSchwarzschild: return f.kind != KIND_SCHWARZSCHILD;
    case Is::Dump: return f.dump;
    case Is::Persistent: return f.variant == 0;
    case Is::Unfused: return !f.fuse_shade;
    case Is::UnfusedNoDump: return !f.fuse_shade && !f.dump;
  }
  return false;
}
/* where in a call a refusal is acted on; callers can tell the order on doubly-wrong calls, so it is part of the contract */
enum At {
  AT_ENTRY, /* before the call's arguments are looked at */
  AT_SHAPE, /* once it is known whether a frame moves; before the refusals all three renderers share (prepare_call_shape) */
  AT_KIND   /* after the metric's validation */
};
struct Refusal {
  At at;
  Is feature, shape;
  const char *message; /* nullptr: the combination exists, the row stands for the record */
};
/* In order of precedence: the first row both of whose facts hold, and that has a message, refuses the call (CURVIS_E_INVALID).
 * A disc and a moving camera live in the fused static kernel alone.  Only the fused kernels hold the mip-mapped and the filtered
 * lookup, the projections and the tile-local resolve: the three staged shapes -- the debug dump, variant = 0, fuse_shade = 0 --
 * are refused under the name of the first of these options that is on.  The scaled steps and the Heun step exist in the fused
 * kernels and in the debug dump's (StagedAdapt), with fuse_shade = 0 or without. */
constexpr Refusal kRefusals[] = {
    {AT_ENTRY, Is::Disc, Is::Dump, "a disc is set: the debug dump shades from the ray store, which has no slot for a disc colour (remove the disc: curvis_ctx_set_disc with rgba = NULL)"},
    {AT_ENTRY, Is::Disc, Is::Persistent, "a disc is set: variant = 0 (the persistent kernel) shades from the ray store, which has no slot for a disc colour"},
    {AT_ENTRY, Is::Disc, Is::Unfused, "a disc is set: fuse_shade = 0 shades from the ray store, which has no slot for a disc colour"},
    {AT_ENTRY, Is::DiscMotion, Is::NotSchwarzschild, "the disc motion is Keplerian and needs the Schwarzschild metric: in the other kinds g00 = -1, free matter is at rest and nothing orbits (set the motion to 0: curvis_ctx_set_disc_motion)"},

    {AT_SHAPE, Is::Moving, Is::Dump, "camera velocity: the debug dump replays the static camera (clear the velocities: curvis_ctx_set_camera_velocities with n = 0)"},
    {AT_SHAPE, Is::Moving, Is::Persistent, "camera velocity: variant = 0 (the persistent kernel) has the static camera only"},
    {AT_SHAPE, Is::Moving, Is::Unfused, "camera velocity: fuse_shade = 0 (the unfused static kernel) has the static camera only"},
    {AT_SHAPE, Is::Moving, Is::DiscMotion, "camera velocity: the emission shift of a moving disc takes the camera to be at rest (set the disc's motion to 0, or clear the velocities)"},

    {AT_SHAPE, Is::Mipmap, Is::Dump, "sky_mipmap = 1: the debug dump records the nearest lookup (set sky_mipmap = 0)"},
    {AT_SHAPE, Is::Projection, Is::Dump, "projection != 0: the debug dump replays the perspective camera (set projection = 0)"},
    {AT_SHAPE, Is::Filter, Is::Dump, "sky_filter = 1: the debug dump records the nearest lookup (set sky_filter = 0)"},
    {AT_SHAPE, Is::Supersample, Is::Dump, "supersample > 1: the debug dump has one record per ray, not per pixel (set supersample = 1)"},
    {AT_SHAPE, Is::StepScale, Is::Dump, nullptr},
    {AT_SHAPE, Is::Integrator, Is::Dump, nullptr},

    {AT_SHAPE, Is::Mipmap, Is::Persistent, "sky_mipmap = 1: variant = 0 (the persistent kernel) shades from the ray store, which has the nearest lookup only"},
    {AT_SHAPE, Is::Projection, Is::Persistent, "projection != 0: variant = 0 (the persistent kernel) has the perspective camera only"},
    {AT_SHAPE, Is::Filter, Is::Persistent, "sky_filter = 1: variant = 0 (the persistent kernel) shades from the ray store, which has the nearest lookup only"},
    {AT_SHAPE, Is::Supersample, Is::Persistent, "supersample > 1: variant = 0 (the persistent kernel) stages single rays and has no tile-local resolve"},
    {AT_SHAPE, Is::StepScale, Is::Persistent, "step_scale != 0: variant = 0 (the persistent kernel) takes the reference's fixed step only"},
    {AT_SHAPE, Is::Integrator, Is::Persistent, "integrator = 1: variant = 0 (the persistent kernel) takes the reference's Euler step only"},

    {AT_SHAPE, Is::Mipmap, Is::Unfused, "sky_mipmap = 1: fuse_shade = 0 shades from the ray store, which has the nearest lookup only"},
    {AT_SHAPE, Is::Projection, Is::Unfused, "projection != 0: fuse_shade = 0 (the unfused static kernel) has the perspective camera only"},
    {AT_SHAPE, Is::Filter, Is::Unfused, "sky_filter = 1: fuse_shade = 0 shades from the ray store, which has the nearest lookup only"},
    {AT_SHAPE, Is::Supersample, Is::Unfused, "supersample > 1: fuse_shade = 0 shades single rays from the ray store and has no tile-local resolve"},
    {AT_SHAPE, Is::StepScale, Is::UnfusedNoDump, "step_scale != 0: fuse_shade = 0 (the unfused static kernel) takes the reference's fixed step only outside the debug dump"},
    {AT_SHAPE, Is::Integrator, Is::UnfusedNoDump, "integrator = 1: fuse_shade = 0 (the unfused static kernel) takes the reference's Euler step only outside the debug dump"},

    {AT_KIND, Is::Schwarzschild, Is::Persistent, "Schwarzschild metric: variant = 0 (the persistent kernel) is not built for this kind (set variant = -1, 1 or 2: the static kernel renders it)"},
};
/* What never takes the relay kernel; the static kernel renders it, and nothing is refused.  There is no relay form of the DISC
 * kernels, of the Schwarzschild kind (its captured rays run ten times the steps of the others, a pattern the hand-over was never
 * tuned on), of the Heun step, or of the mip-mapped lookup (the epilogue is not where a single frame's time goes); a moving camera
 * lives in the static kernel's prologue; and the relay segments are sized in fixed-delta steps, which scaled steps are not. */
constexpr Is kNoRelay[] = {Is::Moving, Is::Disc, Is::Schwarzschild, Is::StepScale, Is::Integrator, Is::Mipmap};

/* ---- the plan ---------------------------------------------------------------------------------------------------------------- */
struct Plan {
  const char *refusal = nullptr; /* CURVIS_E_INVALID with this message, to be acted on at `at`; else the three below */
  At at = AT_ENTRY;
  bool fused = false;            /* the kernel shades in its epilogue: no ray store, no shade launch */
  bool relay = false;            /* the relay kernel (then fused) */
  Family family = Family::Fused;
};
constexpr Plan plan(const Facts &f) {
  Plan p;
  for (const Refusal &r : kRefusals)
    if (r.message && holds(f, r.feature) && holds(f, r.shape)) {
      p.refusal = r.message;
      p.at = r.at;
      return p;
    }
  p.fused = f.variant != 0 && f.fuse_shade && !f.dump;
  p.relay = (f.variant == 2 || f.variant < 0) && p.fused && f.relay_size_ok;
  for (const Is w : kNoRelay)
    if (holds(f, w)) p.relay = false;
  const bool adapt = launch_shape(f).adapt != 0;
  if (f.disc != DISC_NONE) /* phi is integrated by the DISC kernels, and for the debug dump */
    p.family = f.disc == DISC_MOVING ? Family::DiscMotion : Family::Disc;
  else if (f.dump)
    p.family = adapt ? Family::StagedAdapt : f.variant == 0 ? Family::Persistent : Family::Unfused;
  else if (p.relay)
    p.family = Family::Relay;
  else if (adapt)
    p.family = Family::Fused;
  else
    p.family = f.variant == 0 ? Family::Persistent : !p.fused ? Family::Unfused : Family::Fused;
  return p;
}

}  // namespace brute
