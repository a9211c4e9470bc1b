/* cli_args.h -- part of the `curvis` binary (host/curvis_cli.cpp includes the parts in order; one translation unit):
 * command line (src/cli.rs:35-122), the inputs every subcommand shares, context creation, the two render calls. */
#ifndef CURVIS_CLI_ARGS_H
#define CURVIS_CLI_ARGS_H

namespace {

/* ------------------------------------------------------------------ command line */
struct Args {
  std::string sub, bg1, bg2, out, image_toml, video_toml, metric_toml, camera_toml, sim_toml, mode = "efficient", stats,
      sky_broadcast = "rccl";
  bool sky_broadcast_explicit = false, resume = false;
  bool contexts_auto = false; /* --contexts-per-device 0 / not given: video_main may lower the count for short videos */
  int contexts = 0; /* 0 = automatic (4 in --mode efficient, else 1); video: contexts (= host worker threads) per device: while one waits on the host-side sampler or the D2H copy another's kernels run */
  int devices = 1, device = 0, batch = 0, writers = 0; /* batch 0 = automatic (video: 8 frames per launch, in --mode efficient up to 32: cli_video.h); writers 0 = automatic: a quarter of the host's threads, 4..64 */
  int png_level = -1; /* -1 = the fast PNG writer (png_io.h; the reference's image crate also saves with its fast setting), 0..9 = zlib */
  int encode_bench = 0; /* video, diagnostics: every rendered frame is encoded this many extra times into a scratch file */
  std::string gpu_png = "auto"; /* video: PNG front end on the device (curvis_ctx_deflate_frames): auto = with the fast writer, on, off */
  int supersample = 1; /* rays per pixel and axis, averaged on the device (library option "supersample"): 1, 2, 4 or 8 */
  int sky_filter = 0; /* sky lookup (library option "sky_filter"): 0 nearest texel, 1 bilinear */
  int sky_mipmap = 0; /* --sky-mipmap on|off (library option "sky_mipmap"): the bilinear lookup on a mip pyramid of the sky, on top of --sky-filter bilinear */
  int projection = 0; /* pixel -> direction (library option "projection"): 0 perspective, 1 equirectangular, 2 fisheye */
  long long step_scale = 0; /* --step-scale L0 as library option "step_scale" = 256 L0: 0 off, else the Euler step grows as |l| / L0 outside L0 */
  int integrator = 0; /* --integrator euler|heun (library option "integrator"): 0 forward Euler, 1 Heun's method, two Euler steps averaged */
  std::string disc; /* --disc FILE --disc-inner L --disc-outer L: an accretion disc (curvis_ctx_set_disc) textured with the image FILE between
                       the radial coordinates L; all three or none, and --mode brute, the one renderer that sees it */
  std::string disc_inner_s, disc_outer_s;
  double disc_inner = 0.0, disc_outer = 0.0;
  std::string disc_motion_s, disc_gain_s; /* --disc-motion static|prograde|retrograde --disc-gain G: the disc's emission shift
                                             (curvis_ctx_set_disc_motion); with --disc only, a motion only under a metric file with `mass` */
  int disc_motion = 0;
  double disc_gain = 1.0;
  std::string camera_velocity_s; /* image: --camera-velocity BL,BTH,BPH, the camera's velocity in units of c (curvis_ctx_set_camera_velocities) */
  double camera_velocity[3] = {0.0, 0.0, 0.0};
  std::string camera_motion = "static", light_speed_s; /* video: --camera-motion static|path --light-speed C: every frame's velocity from the
                                                          path (curvis_camera_path_velocity), C path units per unit of path time */
  double light_speed = 1.0;
};
/* the disc of the run (Args::disc, decoded by load_common) for make_ctx_bare: every context gets it */
struct DiscOfRun {
  bool set = false;
  pngio::Image img;
  double l_inner = 0.0, l_outer = 0.0;
  int motion = 0;
  double gain = 1.0;
} g_disc;
int g_supersample = 1; /* Args::supersample for make_ctx_bare: every context of the run gets it */
int g_sky_filter = 0;  /* Args::sky_filter, likewise */
int g_sky_mipmap = 0;  /* Args::sky_mipmap, likewise */
int g_projection = 0;  /* Args::projection, likewise */
long long g_step_scale = 0; /* Args::step_scale, likewise */
int g_integrator = 0;  /* Args::integrator, likewise */
bool g_camera_velocity_set = false; /* Args::camera_velocity (`curvis image`), likewise */
double g_camera_velocity[3] = {0.0, 0.0, 0.0};
[[noreturn]] void die(const std::string &msg, int code = 1) {
  std::fprintf(stderr, "%s\n", msg.c_str());
  std::exit(code);
}
void usage() {
  std::printf(
      "Usage: curvis <COMMAND>\n\nCommands:\n  image   renders a single image frame\n  video   renders a video\n"
      "  custom  runs the custom script\n\n"
      "curvis image <IMAGE FILE 1> <IMAGE FILE 2> [OUTPUT FOLDER] [-i|--image-settings <TOML FILE>]\n"
      "curvis video <IMAGE FILE 1> <IMAGE FILE 2> [OUTPUT FOLDER] [-v|--video-settings <TOML FILE>]\n"
      "  common: [-m|--metric-settings <TOML FILE>] [-c|--camera-settings <TOML FILE>] [-s|--simulation-settings <TOML FILE>]\n"
      "  extensions: [--mode efficient|brute|direct] [--device N] [--devices N] [--batch B] [--stats FILE]\n"
      "              [--sky-broadcast rccl|upload] [--writers T] [--resume] [--png-level -1..9] [--gpu-png auto|on|off]\n"
      "              [--contexts-per-device C] [--supersample 1|2|4|8] [--sky-filter nearest|bilinear]\n"
      "              [--projection perspective|equirectangular|fisheye] [--step-scale L0]\n"
      "              [--integrator euler|heun] [--sky-mipmap on|off]\n"
      "              [--disc <IMAGE FILE> --disc-inner L --disc-outer L]  (an accretion disc; needs --mode brute)\n"
      "              [--disc-motion static|prograde|retrograde] [--disc-gain G]  (with --disc; a motion needs a metric file with `mass`)\n"
      "              image: [--camera-velocity BL,BTH,BPH]  (the camera moves: aberration; units of c)\n"
      "              video: [--camera-motion static|path] [--light-speed C]  (every frame's velocity from the camera path)\n");
}
Args parse_args(int argc, char **argv) {
  Args a;
  if (argc < 2) {
    usage();
    die("Subcommand not found");
  }
  a.sub = argv[1];
  if (a.sub == "selftest-png") return a;
  if (a.sub == "-h" || a.sub == "--help") {
    usage();
    std::exit(0);
  }
  std::vector<std::string> pos;
  for (int i = 2; i < argc; ++i) {
    std::string s = argv[i], val;
    auto take = [&](std::string &dst) {
      const size_t eq = s.find('=');
      if (s.rfind("--", 0) == 0 && eq != std::string::npos)
        dst = s.substr(eq + 1);
      else if (i + 1 < argc)
        dst = argv[++i];
      else
        die("error: a value is required for '" + s + "' but none was supplied", 2);
    };
    const std::string key = s.substr(0, s.find('='));
    if (key == "-i" || key == "--image-settings") take(a.image_toml);
    else if (key == "-v" || key == "--video-settings") take(a.video_toml);
    else if (key == "-m" || key == "--metric-settings") take(a.metric_toml);
    else if (key == "-c" || key == "--camera-settings") take(a.camera_toml);
    else if (key == "-s" || key == "--simulation-settings") take(a.sim_toml);
    else if (key == "--mode") take(a.mode);
    else if (key == "--stats") take(a.stats);
    else if (key == "--sky-broadcast") { take(a.sky_broadcast); a.sky_broadcast_explicit = true; }
    else if (key == "--resume") a.resume = true;
    else if (key == "--devices") { take(val); a.devices = std::atoi(val.c_str()); }
    else if (key == "--contexts-per-device") { take(val); a.contexts = std::max(0, std::min(8, std::atoi(val.c_str()))); }
    else if (key == "--device") { take(val); a.device = std::atoi(val.c_str()); }
    else if (key == "--batch") { take(val); a.batch = std::atoi(val.c_str()); }
    else if (key == "--writers") { take(val); a.writers = std::atoi(val.c_str()); }
    else if (key == "--png-level") { take(val); a.png_level = std::max(-1, std::min(9, std::atoi(val.c_str()))); }
    else if (key == "--encode-bench") { take(val); a.encode_bench = std::max(0, std::atoi(val.c_str())); }
    else if (key == "--gpu-png") take(a.gpu_png);
    else if (key == "--supersample") {
      take(val);
      if (val != "1" && val != "2" && val != "4" && val != "8") die("error: --supersample must be 1, 2, 4 or 8", 2);
      a.supersample = g_supersample = std::atoi(val.c_str());
    }
    else if (key == "--sky-filter") {
      take(val);
      if (val != "nearest" && val != "bilinear") die("error: --sky-filter must be nearest or bilinear", 2);
      a.sky_filter = g_sky_filter = val == "bilinear" ? 1 : 0;
    }
    else if (key == "--sky-mipmap") {
      take(val);
      if (val != "on" && val != "off") die("error: --sky-mipmap must be on or off", 2);
      a.sky_mipmap = g_sky_mipmap = val == "on" ? 1 : 0;
    }
    else if (key == "--projection") {
      take(val);
      if (val != "perspective" && val != "equirectangular" && val != "fisheye")
        die("error: --projection must be perspective, equirectangular or fisheye", 2);
      a.projection = g_projection = val == "fisheye" ? 2 : val == "equirectangular" ? 1 : 0;
    }
    else if (key == "--step-scale") { /* a decimal number L0, a multiple of 1/256 in [0, 4096]: 256 L0 is the library's integer */
      take(val);
      char *end = nullptr;
      /* digits, one point, an optional exponent: no sign, no blank, no hexadecimal or named value of strtod's */
      const bool decimal = !val.empty() && val.find_first_not_of("0123456789.eE+-") == std::string::npos &&
                           ((val[0] >= '0' && val[0] <= '9') || val[0] == '.');
      const double l0 = decimal ? std::strtod(val.c_str(), &end) : -1.0;
      const double scaled = l0 * 256.0;
      if (!decimal || *end != '\0' || !(scaled >= 0.0) || scaled > 1048576.0 || scaled != (double)(long long)scaled)
        die("error: --step-scale must be 0 or a multiple of 1/256 up to 4096", 2);
      a.step_scale = g_step_scale = (long long)scaled;
    }
    else if (key == "--integrator") {
      take(val);
      if (val != "euler" && val != "heun") die("error: --integrator must be euler or heun", 2);
      a.integrator = g_integrator = val == "heun" ? 1 : 0;
    }
    else if (key == "--camera-velocity") take(a.camera_velocity_s);
    else if (key == "--camera-motion") take(a.camera_motion);
    else if (key == "--light-speed") take(a.light_speed_s);
    else if (key == "--disc") take(a.disc);
    else if (key == "--disc-inner") take(a.disc_inner_s);
    else if (key == "--disc-outer") take(a.disc_outer_s);
    else if (key == "--disc-motion") take(a.disc_motion_s);
    else if (key == "--disc-gain") take(a.disc_gain_s);
    else if (key == "-h" || key == "--help") { usage(); std::exit(0); }
    else if (!s.empty() && s[0] == '-') die("error: unexpected argument '" + s + "' found", 2);
    else pos.push_back(s);
  }
  if (a.sub == "image" || a.sub == "video") {
    /* one image alone is a complete command under a Schwarzschild metric file (load_common: the -l background is then black) */
    if (pos.size() < 2 && (pos.empty() || a.metric_toml.empty())) die("error: the following required arguments were not provided:\n  <IMAGE FILE 1>\n  <IMAGE FILE 2>", 2);
    if (pos.size() > 3) die("error: unexpected argument '" + pos[3] + "' found", 2);
    a.bg1 = pos[0];
    if (pos.size() >= 2) a.bg2 = pos[1];
    if (pos.size() == 3) a.out = pos[2];
    if (a.sub == "image" && !a.video_toml.empty()) die("error: unexpected argument '-v' found", 2);
    if (a.sub == "video" && !a.image_toml.empty()) die("error: unexpected argument '-i' found", 2);
  }
  if (a.mode != "efficient" && a.mode != "brute" && a.mode != "direct") die("error: --mode must be efficient, brute or direct", 2);
  if (!a.disc.empty() || !a.disc_inner_s.empty() || !a.disc_outer_s.empty()) {
    if (a.disc.empty() || a.disc_inner_s.empty() || a.disc_outer_s.empty())
      die("error: --disc, --disc-inner and --disc-outer are given together, or none of them", 2);
    auto number = [](const std::string &v, double &out) {
      char *end = nullptr;
      out = std::strtod(v.c_str(), &end);
      return !v.empty() && *end == '\0' && std::isfinite(out);
    };
    if (!number(a.disc_inner_s, a.disc_inner) || !number(a.disc_outer_s, a.disc_outer) || !(a.disc_inner < a.disc_outer))
      die("error: --disc-inner and --disc-outer must be finite numbers, the inner one less than the outer", 2);
    /* no silent change of mode: the efficient and the direct renderer reduce every ray to an equatorial orbit and cannot see a disc */
    if (a.mode != "brute") die("error: --disc needs --mode brute (the per-pixel renderer is the one that sees a disc); this run is --mode " + a.mode, 2);
  }
  if (!a.disc_motion_s.empty() || !a.disc_gain_s.empty()) {
    if (a.disc.empty()) die("error: --disc-motion and --disc-gain need --disc (they say how the disc emits)", 2);
    if (!a.disc_motion_s.empty()) {
      if (a.disc_motion_s != "static" && a.disc_motion_s != "prograde" && a.disc_motion_s != "retrograde")
        die("error: --disc-motion must be static, prograde or retrograde", 2);
      a.disc_motion = a.disc_motion_s == "prograde" ? 1 : a.disc_motion_s == "retrograde" ? -1 : 0;
    }
    if (!a.disc_gain_s.empty()) {
      char *end = nullptr;
      a.disc_gain = std::strtod(a.disc_gain_s.c_str(), &end);
      if (*end != '\0' || !std::isfinite(a.disc_gain) || a.disc_gain < 0.0) die("error: --disc-gain must be a finite number, not negative", 2);
    }
  }
  if (!a.camera_velocity_s.empty()) {
    if (a.sub != "image") die("error: --camera-velocity belongs to `curvis image` (a video takes --camera-motion path)", 2);
    char *end = nullptr;
    const char *p = a.camera_velocity_s.c_str();
    bool ok = true;
    for (int i = 0; i < 3 && ok; ++i) {
      a.camera_velocity[i] = std::strtod(p, &end);
      ok = end != p && *end == (i < 2 ? ',' : '\0');
      p = end + 1;
    }
    const double *b = a.camera_velocity;
    if (!ok || !((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2] < 1.0))
      die("error: --camera-velocity must be BL,BTH,BPH, three numbers with a speed below 1 (the speed of light)", 2);
    g_camera_velocity_set = true;
    for (int i = 0; i < 3; ++i) g_camera_velocity[i] = b[i];
  }
  if (a.camera_motion != "static" && a.camera_motion != "path") die("error: --camera-motion must be static or path", 2);
  if (a.camera_motion != "static" && a.sub != "video") die("error: --camera-motion belongs to `curvis video` (an image takes --camera-velocity)", 2);
  if (!a.light_speed_s.empty()) {
    char *end = nullptr;
    a.light_speed = std::strtod(a.light_speed_s.c_str(), &end);
    if (*end != '\0' || !std::isfinite(a.light_speed) || !(a.light_speed > 0.0)) die("error: --light-speed must be a positive number", 2);
    if (a.camera_motion != "path") die("error: --light-speed needs --camera-motion path", 2);
  }
  if (a.sky_broadcast != "rccl" && a.sky_broadcast != "upload") die("error: --sky-broadcast must be rccl or upload", 2);
  if (a.gpu_png != "auto" && a.gpu_png != "on" && a.gpu_png != "off") die("error: --gpu-png must be auto, on or off", 2);
  if (a.devices < 1) a.devices = 1;
  /* --mode efficient spends more than half of a frame's render call on the host (the adaptive sampler between its launches of
   * lone waves) and its kernels do not fill the GPU: several contexts per GPU overlap one's host work and another's kernels, and
   * the kernels of different contexts run side by side.  Measured at 30 000 frames per cell on one MI355X, 32 frames per launch
   * (profiles/round5_eff_contexts_sweep.txt): 2 757 / 4 058 / 5 488 / 6 116 / 5 936 1080p frames/s with 1 / 2 / 3 / 4 / 6 contexts.
   * The per-pixel modes keep the GPU busy by themselves. */
  /* CPUs this process may really use: a container may see every CPU of the host behind a much smaller cgroup quota
   * ("1600000 100000" = 16 CPUs) */
  unsigned hw = std::max(1u, std::thread::hardware_concurrency()), cpus = hw;
  if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    double quota = 0.0, period = 0.0;
    if (std::fscanf(f, "%lf %lf", &quota, &period) == 2 && quota > 0.0 && period > 0.0) {
      cpus = std::max(1u, std::min(hw, (unsigned)(quota / period + 0.5)));
      hw = std::min(hw, cpus * 4u); /* the quota itself: this many writers at most */
    }
    std::fclose(f);
  }
  /* up to six contexts per GPU in --mode efficient (four below 12 000 frames per GPU, see video_main) -- as far as the host has two CPUs per worker thread (each context's thread runs
   * the sampler's host side; 8 GPUs behind a 16-CPU quota get one context each, not 32 threads fighting the writers) */
  a.contexts_auto = a.contexts == 0;
  if (a.contexts == 0) a.contexts = a.mode == "efficient" ? (int)std::max(1u, std::min(6u, cpus / (2u * (unsigned)a.devices))) : 1; /* video_main: fewer for shorter videos */
  if (a.batch < 0) a.batch = 0;
  if (a.writers < 1) /* encoding a 1080p frame costs 5-25 ms of a host thread (zlib: 20-230): the GPU renders one in 0.4-10 ms */
    a.writers = (int)std::min(64u, std::max(4u, hw / 4u));
  return a;
}

/* CURVIS_DEBUG_TIMING=1: the phases of a run on stderr (settings, background images, contexts, render, save) */
struct PhaseClock {
  const bool on = std::getenv("CURVIS_DEBUG_TIMING") != nullptr;
  double t0 = pngio::now_s(), last = t0;
  void mark(const char *what) {
    if (!on) return;
    const double t = pngio::now_s();
    std::fprintf(stderr, "[curvis timing] %-34s %8.1f ms  (at %8.1f ms)\n", what, (t - last) * 1e3, (t - t0) * 1e3);
    last = t;
  }
};

struct Common {
  curvis_metric metric{CURVIS_METRIC_ELLIS, 0, 1.0, 0.0, 0.0}; /* default: Ellis rho = 1 (ellis_metric_settings.toml) */
  CameraSettings cam;
  SimulationSettings sim;
  pngio::Image sky1, sky2;
  std::string out;
};

void load_common(const Args &a_in, Common &c, const char *what) {
  std::string err;
  auto need = [&](const std::string &f, const char *label) {
    if (!path_exists(f)) die(std::string("Error with ") + label + ": File \"" + f + "\" not found.");
  };
  Args a = a_in;
  need(a.bg1, "background image 1");
  /* under a Schwarzschild metric (a metric file with `mass`) the second background is "what is painted on the horizon" and may be left
   * out -- `curvis image <IMAGE FILE 1> [<OUTPUT FOLDER>] -m <mass file>` -- for an opaque black 1 x 1 image */
  bool hole = false; /* a look ahead only: errors of the metric file are reported below, in the order they always were */
  if (!a.metric_toml.empty() && path_exists(a.metric_toml)) {
    curvis_metric peek{};
    std::string ignored;
    hole = metric_from_toml(a.metric_toml, peek, ignored) && peek.kind == CURVIS_METRIC_SCHWARZSCHILD;
  }
  if (hole && a.out.empty() && !a.bg2.empty() && is_dir(a.bg2)) a.out = a.bg2, a.bg2.clear();
  if (a.bg2.empty() && !hole) die("error: the following required arguments were not provided:\n  <IMAGE FILE 2>", 2);
  const bool black_horizon = a.bg2.empty();
  if (!black_horizon) need(a.bg2, "background image 2");
  if (a.out.empty()) {
    char cwd[4096];
    if (!::getcwd(cwd, sizeof cwd)) die("Error with output folder: Could not get current working directory.");
    c.out = cwd;
  } else {
    if (!path_exists(a.out)) die("Error with output folder: File \"" + a.out + "\" not found.");
    if (!is_dir(a.out)) die("Error with output folder: \"" + a.out + "\" is not a folder.");
    c.out = a.out;
  }
  if (!a.metric_toml.empty()) {
    need(a.metric_toml, "metric settings");
    if (!metric_from_toml(a.metric_toml, c.metric, err)) die("Error with metric settings: " + err);
  }
  if (!a.camera_toml.empty()) {
    need(a.camera_toml, "camera settings");
    if (!from_toml(a.camera_toml, c.cam, err)) die("Error with camera settings: " + err);
  }
  if (!a.sim_toml.empty()) {
    need(a.sim_toml, "simulation settings");
    if (!from_toml(a.sim_toml, c.sim, err)) die("Error with simulation settings: " + err);
  }
  /* instantiate_metric (src/main.rs:114-132): constructor panics */
  if (curvis_metric_validate(&c.metric) != CURVIS_OK)
    die(std::string("Error in rendering ") + what + ": metric parameters must be positive (src/metrics.rs:409-456)", 101);
  if (!validate(c.cam, err) || !validate(c.sim, err)) die(std::string("Error in rendering ") + what + ": " + err);
  /* a disc's motion is Keplerian: a hole only (the library refuses the render call; this says so before anything is decoded) */
  if (a.disc_motion != 0 && c.metric.kind != CURVIS_METRIC_SCHWARZSCHILD)
    die("error: --disc-motion " + a.disc_motion_s + " needs a metric file with `mass` (-m: a Schwarzschild hole); in the other metrics free matter is at rest and nothing orbits", 2);
  /* both backgrounds are decoded at the same time (an 8192x4096 PNG takes the better part of a second to inflate and
   * unfilter); errors are reported in the reference's order, image 1 first */
  std::string err2;
  bool ok2 = false;
  /* the HIP runtime comes up (hipInit, behind curvis_device_count) while the backgrounds are decoded: the two slow each other
   * down -- the decode 90 -> 150 ms, the runtime's start-up 70 -> ~110 -- and still finish 10-25 ms sooner than one after the
   * other (251 -> 235 ms per `curvis image`; CURVIS_NO_EARLY_INIT=1 switches it off) */
  std::thread early_init;
  if (!std::getenv("CURVIS_NO_EARLY_INIT")) {
    try {
      early_init = std::thread([] { (void)curvis_device_count(); });
    } catch (const std::exception &) {
    }
  }
  struct JoinEarly {
    std::thread &t;
    ~JoinEarly() { if (t.joinable()) t.join(); }
  } join_early{early_init};
  std::thread second([&] {
    if (black_horizon) {
      c.sky2.w = c.sky2.h = 1;
      c.sky2.rgba = {0, 0, 0, 255};
      ok2 = true;
    } else {
      ok2 = jpegio::load_image(a.bg2, c.sky2, err2);
    }
  });
  const bool ok1 = jpegio::load_image(a.bg1, c.sky1, err);
  second.join();
  /* die() is std::exit(): it does not unwind, so JoinEarly would never run, and exit()'s handlers / the static destructors of
   * libamdhip64 would tear the runtime down while hipInit is still executing on the helper thread (a decode error returns in
   * microseconds, hipInit takes ~100 ms) -- join it first, the error path is not the fast path */
  if ((!ok1 || !ok2) && early_init.joinable()) early_init.join();
  if (!ok1) die(std::string("Error in rendering ") + what + ": background image 1: " + err);
  if (!ok2) die(std::string("Error in rendering ") + what + ": background image 2: " + err2);
  if (!a.disc.empty()) {
    if (early_init.joinable()) early_init.join(); /* as above: die() must not race hipInit */
    need(a.disc, "disc image");
    if (!jpegio::load_image(a.disc, g_disc.img, err)) die(std::string("Error in rendering ") + what + ": disc image: " + err);
    g_disc.l_inner = a.disc_inner, g_disc.l_outer = a.disc_outer;
    g_disc.motion = a.disc_motion, g_disc.gain = a.disc_gain;
    g_disc.set = true;
  }
}

void check(int rc, curvis_ctx *ctx, const char *what) {
  if (rc == CURVIS_OK) return;
  const char *msg = curvis_last_error(ctx);
  die(std::string("Error in rendering ") + what + ": " + (msg ? msg : "") + " (code " + std::to_string(rc) + ")",
      (rc == CURVIS_E_CAMERA_OUTSIDE || rc == CURVIS_E_PARALLEL || rc == CURVIS_E_SAMPLING) ? 101 : 1);
}

curvis_ctx *make_ctx_bare(int device, const char *what) {
  curvis_ctx *ctx = nullptr;
  int rc = curvis_ctx_create(device, &ctx);
  if (rc != CURVIS_OK) die(std::string("Error in rendering ") + what + ": " + curvis_last_error(nullptr));
  /* tuning knobs of the library for experiments (tools/gpu_eff_speculation_sweep.py): CURVIS_CTX_OPTIONS="key=value,key=value"
   * is applied to every context of the run; an unknown key is an error, not a silent no-op */
  if (const char *opts = std::getenv("CURVIS_CTX_OPTIONS")) {
    std::stringstream ss(opts);
    std::string kv;
    while (std::getline(ss, kv, ',')) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || curvis_ctx_set_option(ctx, kv.substr(0, eq).c_str(), std::atoll(kv.c_str() + eq + 1)) != CURVIS_OK)
        die("error: CURVIS_CTX_OPTIONS: cannot set `" + kv + "`", 2);
    }
  }
  if (g_supersample != 1) check(curvis_ctx_set_option(ctx, "supersample", g_supersample), ctx, what);
  if (g_sky_filter != 0) check(curvis_ctx_set_option(ctx, "sky_filter", g_sky_filter), ctx, what);
  if (g_sky_mipmap != 0) check(curvis_ctx_set_option(ctx, "sky_mipmap", g_sky_mipmap), ctx, what);
  if (g_projection != 0) check(curvis_ctx_set_option(ctx, "projection", g_projection), ctx, what);
  if (g_step_scale != 0) check(curvis_ctx_set_option(ctx, "step_scale", g_step_scale), ctx, what);
  if (g_integrator != 0) check(curvis_ctx_set_option(ctx, "integrator", g_integrator), ctx, what);
  if (g_disc.set) check(curvis_ctx_set_disc(ctx, g_disc.img.rgba.data(), g_disc.img.w, g_disc.img.h, g_disc.l_inner, g_disc.l_outer), ctx, what);
  if (g_disc.set && (g_disc.motion != 0 || g_disc.gain != 1.0)) check(curvis_ctx_set_disc_motion(ctx, g_disc.motion, g_disc.gain), ctx, what);
  if (g_camera_velocity_set) check(curvis_ctx_set_camera_velocities(ctx, g_camera_velocity, 1), ctx, what);
  return ctx;
}
void upload_skies(curvis_ctx *ctx, const Common &c, const char *what) {
  check(curvis_ctx_set_sky(ctx, 0, c.sky1.rgba.data(), c.sky1.w, c.sky1.h), ctx, what);
  check(curvis_ctx_set_sky(ctx, 1, c.sky2.rgba.data(), c.sky2.w, c.sky2.h), ctx, what);
}
curvis_ctx *make_ctx(int device, const Common &c, const char *what) {
  curvis_ctx *ctx = make_ctx_bare(device, what);
  upload_skies(ctx, c, what);
  return ctx;
}

/* the sampler of a batch that render_frames will render later, started now (efficient mode; curvis_ctx_prefetch_efficient is a
 * no-op where the library would not sample on the device).  Failures are not fatal: the render call then samples itself. */
void prefetch_frames(curvis_ctx *ctx, const Args &a, const Common &c, const curvis_camera *cams, uint32_t n, double thr2) {
  if (a.mode != "efficient" || n == 0) return;
  (void)curvis_ctx_prefetch_efficient(ctx, &c.metric, cams, n, c.sim.ray_integration_max_itarations, c.sim.escape_radius,
                                      c.sim.ray_integration_step, c.sim.sampling_initial_nums, c.sim.sampling_initial_nums,
                                      c.sim.sampling_convergence_threshold_1, thr2);
}

/* per-frame statistics of the last render_frames call of this thread in "direct" mode (one render call per frame there;
 * the batch calls of the other modes keep theirs inside the context: curvis_ctx_frame_stats) */
thread_local std::vector<curvis_stats> g_direct_frame_stats;

/* beta (video, --camera-motion path): the n frames' velocities, set on the context before the call that renders them */
int render_frames(curvis_ctx *ctx, const Args &a, const Common &c, const curvis_camera *cams, uint32_t n, double thr2,
                  uint8_t *rgb, curvis_stats *st, const double *beta = nullptr) {
  if (beta && a.mode != "direct")
    if (const int rc = curvis_ctx_set_camera_velocities(ctx, beta, n)) return rc;
  if (a.mode == "brute")
    return curvis_render_brute_batch(ctx, &c.metric, cams, n, c.sim.ray_integration_max_itarations, c.sim.escape_radius,
                                     c.sim.ray_integration_step, rgb, st);
  if (a.mode == "direct") { /* extension: compute_escape_angle for every pixel, no sampling / interpolation; frame by frame */
    curvis_stats tot;
    std::memset(&tot, 0, sizeof tot);
    const size_t fbytes = (size_t)cams[0].res_x * cams[0].res_y * 3;
    g_direct_frame_stats.clear();
    for (uint32_t f = 0; f < n; ++f) {
      curvis_stats one;
      if (beta)
        if (const int brc = curvis_ctx_set_camera_velocities(ctx, beta + 3 * (size_t)f, 1)) return brc;
      const int rc = curvis_render_direct(ctx, &c.metric, cams + f, c.sim.ray_integration_max_itarations, c.sim.escape_radius,
                                          c.sim.ray_integration_step, rgb + (size_t)f * fbytes, &one);
      if (rc != CURVIS_OK) return rc;
      g_direct_frame_stats.push_back(one);
      tot.rays += one.rays;
      tot.steps += one.steps;
      tot.n_pos += one.n_pos;
      tot.n_neg += one.n_neg;
      tot.n_none += one.n_none;
      tot.n_oob += one.n_oob;
      tot.kernel_ms += one.kernel_ms;
      tot.integrate_ms += one.integrate_ms;
      tot.total_ms += one.total_ms;
    }
    if (st) *st = tot;
    return CURVIS_OK;
  }
  /* src/main.rs:46-47 / :106-107: alphas_num AND max_iterations_sampling both take sampling_initial_nums */
  return curvis_render_efficient_batch(ctx, &c.metric, cams, n, c.sim.ray_integration_max_itarations, c.sim.escape_radius,
                                       c.sim.ray_integration_step, c.sim.sampling_initial_nums, c.sim.sampling_initial_nums,
                                       c.sim.sampling_convergence_threshold_1, thr2, rgb, st);
}

}  // namespace

#endif /* CURVIS_CLI_ARGS_H */
