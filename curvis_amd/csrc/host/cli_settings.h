/* cli_settings.h -- part of the `curvis` binary (host/curvis_cli.cpp includes the parts in order; one translation unit):
 * TOML subset, the six settings groups with their validation (src/settings.rs), the metric file (src/cli.rs:233-261), the camera-path CSV reader and interpolator (src/csv.rs, src/interpolation.rs). */
#ifndef CURVIS_CLI_SETTINGS_H
#define CURVIS_CLI_SETTINGS_H

namespace {

/* ------------------------------------------------------------------ tiny TOML subset (key = value) */
struct TomlValue {
  enum Kind { STRING, INTEGER, FLOAT, BOOLEAN } kind = STRING;
  std::string s;
  long long i = 0;
  double f = 0.0;
};
typedef std::map<std::string, TomlValue> TomlTable;

bool parse_toml(const std::string &text, TomlTable &out, std::string &err) {
  std::istringstream in(text);
  std::string line;
  int ln = 0;
  while (std::getline(in, line)) {
    ++ln;
    /* strip comments outside strings */
    bool in_str = false;
    size_t cut = std::string::npos;
    for (size_t k = 0; k < line.size(); ++k) {
      if (line[k] == '"' && (k == 0 || line[k - 1] != '\\')) in_str = !in_str;
      if (line[k] == '#' && !in_str) {
        cut = k;
        break;
      }
    }
    if (cut != std::string::npos) line.resize(cut);
    auto trim = [](std::string &s) {
      size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
      s = (a == std::string::npos) ? std::string() : s.substr(a, b - a + 1);
    };
    trim(line);
    if (line.empty()) continue;
    if (line[0] == '[') continue; /* tables are not used by the reference's settings */
    const size_t eq = line.find('=');
    if (eq == std::string::npos) {
      err = "line " + std::to_string(ln) + ": expected key = value";
      return false;
    }
    std::string key = line.substr(0, eq), val = line.substr(eq + 1);
    trim(key);
    trim(val);
    if (key.empty() || val.empty()) {
      err = "line " + std::to_string(ln) + ": empty key or value";
      return false;
    }
    TomlValue v;
    if (val[0] == '"' || val[0] == '\'') {
      const char q = val[0];
      const size_t end = val.find_last_of(q);
      if (end == 0) {
        err = "line " + std::to_string(ln) + ": unterminated string";
        return false;
      }
      v.kind = TomlValue::STRING;
      v.s = val.substr(1, end - 1);
    } else if (val == "true" || val == "false") {
      v.kind = TomlValue::BOOLEAN;
      v.i = val == "true";
    } else {
      std::string num;
      for (char ch : val)
        if (ch != '_') num.push_back(ch);
      const bool is_float = num.find_first_of(".eE") != std::string::npos || num == "inf" || num == "nan" ||
                            num == "+inf" || num == "-inf";
      char *endp = nullptr;
      errno = 0;
      if (is_float) {
        v.kind = TomlValue::FLOAT;
        v.f = std::strtod(num.c_str(), &endp);
      } else {
        v.kind = TomlValue::INTEGER;
        v.i = std::strtoll(num.c_str(), &endp, 10);
        v.f = (double)v.i;
      }
      if (!endp || *endp != 0 || errno == ERANGE) {
        err = "line " + std::to_string(ln) + ": invalid value `" + val + "`";
        return false;
      }
    }
    out[key] = v;
  }
  return true;
}

/* serde semantics: missing field = error; an integer deserialises into f64; a float does not into u32 */
bool get_f64(const TomlTable &t, const char *k, double &out, std::string &err) {
  auto it = t.find(k);
  if (it == t.end()) {
    err = std::string("missing field `") + k + "`";
    return false;
  }
  if (it->second.kind != TomlValue::FLOAT && it->second.kind != TomlValue::INTEGER) {
    err = std::string("invalid type for `") + k + "`, expected f64";
    return false;
  }
  out = it->second.f;
  return true;
}
bool get_u32(const TomlTable &t, const char *k, uint32_t &out, std::string &err) {
  auto it = t.find(k);
  if (it == t.end()) {
    err = std::string("missing field `") + k + "`";
    return false;
  }
  if (it->second.kind != TomlValue::INTEGER || it->second.i < 0 || it->second.i > 4294967295LL) {
    err = std::string("invalid type or range for `") + k + "`, expected u32";
    return false;
  }
  out = (uint32_t)it->second.i;
  return true;
}
bool get_str(const TomlTable &t, const char *k, std::string &out, std::string &err) {
  auto it = t.find(k);
  if (it == t.end()) {
    err = std::string("missing field `") + k + "`";
    return false;
  }
  if (it->second.kind != TomlValue::STRING) {
    err = std::string("invalid type for `") + k + "`, expected a string";
    return false;
  }
  out = it->second.s;
  return true;
}

bool read_text(const std::string &path, std::string &out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::ostringstream ss;
  ss << f.rdbuf();
  out = ss.str();
  return true;
}
bool path_exists(const std::string &p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0;
}
bool is_dir(const std::string &p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

/* ------------------------------------------------------------------ settings (src/settings.rs:22-217) */
struct VideoSettings {
  std::string video_name = "output_video";
  double frame_rate = 30.0;
  std::string filepath_to_camera_path = "paths/path_through.csv";
};
struct ImageSettings {
  std::string image_name = "output_image";
  double t = 0.0, l = 5.0, theta = 1.5707963267948966192313216916398, phi = 0.0;
  double forward_x = -1.0, forward_y = 0.0, forward_z = 0.0, up_x = 0.0, up_y = 0.0, up_z = 1.0;
};
struct CameraSettings {
  uint32_t resolution_x = 960, resolution_y = 540;
  double diagonal = 43.0, focal_length = 15.0;
};
struct SimulationSettings {
  double escape_radius = 100.0;
  uint32_t ray_integration_max_itarations = 40000;
  double ray_integration_step = 0.05;
  uint32_t sampling_initial_nums = 100, sampling_max_iterations = 50;
  double sampling_convergence_threshold_1 = 1e-5, sampling_convergence_threshold_2 = 1e-5;
};

std::string package_root() { /* CURVIS_HOME, else the directory two levels above the executable */
  if (const char *h = std::getenv("CURVIS_HOME")) return h;
  char buf[4096];
  ssize_t n = ::readlink("/proc/self/exe", buf, sizeof buf - 1);
  if (n <= 0) return ".";
  buf[n] = 0;
  std::string p(buf);
  for (int k = 0; k < 2; ++k) {
    const size_t s = p.find_last_of('/');
    if (s == std::string::npos) return ".";
    p.resize(s);
  }
  return p; /* .../curvis_amd */
}
std::string resolve_path(const std::string &p) { /* src/filepaths.rs:42-47: relative paths are package-relative */
  if (!p.empty() && p[0] == '/') return p;
  if (path_exists(p)) return p;
  const std::string root = package_root();
  for (const std::string &cand : {root + "/" + p, root + "/data/" + p})
    if (path_exists(cand)) return cand;
  return root + "/" + p;
}
bool has_extension(const std::string &p, const char *ext) {
  const size_t d = p.find_last_of('.');
  return d != std::string::npos && p.substr(d + 1) == ext;
}

bool load_table(const std::string &file, TomlTable &t, std::string &err) {
  if (!has_extension(file, "toml")) {
    err = "The file \"" + file + "\" is not a toml file.";
    return false;
  }
  std::string text;
  if (!read_text(file, text)) {
    err = "Could not read file \"" + file + "\"";
    return false;
  }
  return parse_toml(text, t, err);
}

bool from_toml(const std::string &file, VideoSettings &s, std::string &err) {
  TomlTable t;
  return load_table(file, t, err) && get_str(t, "video_name", s.video_name, err) &&
         get_f64(t, "frame_rate", s.frame_rate, err) && get_str(t, "filepath_to_camera_path", s.filepath_to_camera_path, err);
}
bool from_toml(const std::string &file, ImageSettings &s, std::string &err) {
  TomlTable t;
  return load_table(file, t, err) && get_str(t, "image_name", s.image_name, err) && get_f64(t, "t", s.t, err) &&
         get_f64(t, "l", s.l, err) && get_f64(t, "theta", s.theta, err) && get_f64(t, "phi", s.phi, err) &&
         get_f64(t, "forward_x", s.forward_x, err) && get_f64(t, "forward_y", s.forward_y, err) &&
         get_f64(t, "forward_z", s.forward_z, err) && get_f64(t, "up_x", s.up_x, err) &&
         get_f64(t, "up_y", s.up_y, err) && get_f64(t, "up_z", s.up_z, err);
}
bool from_toml(const std::string &file, CameraSettings &s, std::string &err) {
  TomlTable t;
  return load_table(file, t, err) && get_u32(t, "resolution_x", s.resolution_x, err) &&
         get_u32(t, "resolution_y", s.resolution_y, err) && get_f64(t, "diagonal", s.diagonal, err) &&
         get_f64(t, "focal_length", s.focal_length, err);
}
bool from_toml(const std::string &file, SimulationSettings &s, std::string &err) {
  TomlTable t;
  return load_table(file, t, err) && get_f64(t, "escape_radius", s.escape_radius, err) &&
         get_u32(t, "ray_integration_max_itarations", s.ray_integration_max_itarations, err) &&
         get_f64(t, "ray_integration_step", s.ray_integration_step, err) &&
         get_u32(t, "sampling_initial_nums", s.sampling_initial_nums, err) &&
         get_u32(t, "sampling_max_iterations", s.sampling_max_iterations, err) &&
         get_f64(t, "sampling_convergence_threshold_1", s.sampling_convergence_threshold_1, err) &&
         get_f64(t, "sampling_convergence_threshold_2", s.sampling_convergence_threshold_2, err);
}
/* metric file: tried as Interstellar (m, a, rho) first, then Ellis (rho) -- src/cli.rs:233-261 --, then, a form the reference does not
 * have, Schwarzschild (mass): a file with `mass` and no `rho`.  Every file the first two forms read keeps its meaning. */
bool metric_from_toml(const std::string &file, curvis_metric &m, std::string &err) {
  TomlTable t;
  if (!load_table(file, t, err)) {
    err = "Could not read the metric configuration file.";
    return false;
  }
  std::string e;
  double mm, aa, rho;
  if (get_f64(t, "m", mm, e) && get_f64(t, "a", aa, e) && get_f64(t, "rho", rho, e)) {
    m.kind = CURVIS_METRIC_INTERSTELLAR;
    m.m = mm;
    m.a = aa;
    m.rho = rho;
    return true;
  }
  if (get_f64(t, "rho", rho, e)) {
    m.kind = CURVIS_METRIC_ELLIS;
    m.rho = rho;
    m.m = m.a = 0.0;
    return true;
  }
  double mass;
  if (get_f64(t, "mass", mass, e)) {
    m.kind = CURVIS_METRIC_SCHWARZSCHILD;
    m.m = mass;
    m.rho = m.a = 0.0;
    return true;
  }
  err = "Could not read the metric configuration file.";
  return false;
}

bool validate(const CameraSettings &c, std::string &err) { /* src/settings.rs:98-124 */
  if (c.resolution_x == 0) return err = "The resolution in the x direction must be larger than zero.", false;
  if (c.resolution_y == 0) return err = "The resolution in the y direction must be larger than zero.", false;
  if (c.diagonal <= 0.0) return err = "The diagonal of the camera must be larger than zero.", false;
  if (c.focal_length <= 0.0) return err = "The focal length of the camera must be larger than zero.", false;
  return true;
}
bool validate(const SimulationSettings &s, std::string &err) { /* src/settings.rs:137-174 */
  if (s.escape_radius <= 0.0) return err = "The escape radius must be larger than zero.", false;
  if (s.ray_integration_max_itarations == 0)
    return err = "The maximum number of iterations for the ray integration must be larger than zero.", false;
  if (s.ray_integration_step <= 0.0) return err = "The step for the ray integration must be larger than zero.", false;
  if (s.sampling_initial_nums <= 1) return err = "The initial number of samples must be larger than two.", false;
  if (s.sampling_max_iterations == 0)
    return err = "The maximum number of iterations for the sampling must be larger than zero.", false;
  if (s.sampling_convergence_threshold_1 <= 0.0)
    return err = "The first convergence threshold for the sampling must be larger than zero.", false;
  if (s.sampling_convergence_threshold_2 <= 0.0)
    return err = "The second convergence threshold for the sampling must be larger than zero.", false;
  return true;
}

/* ------------------------------------------------------------------ camera path (src/csv.rs, src/interpolation.rs) */
struct CameraPath {
  std::vector<double> pos, fwd, up; /* n*4, n*3, n*3 */
  size_t n = 0;
};
bool load_path(const std::string &file, CameraPath &p, std::string &err) {
  std::string text;
  if (!read_text(file, text)) return err = "Could not open file", false;
  size_t start = 0, index = 0;
  while (start <= text.size()) {
    size_t end = text.find('\n', start);
    const bool last = end == std::string::npos;
    if (last) end = text.size();
    std::string line = text.substr(start, end - start);
    start = end + 1;
    if (last && line.empty()) break;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (index++ == 0) {
      if (last) break;
      continue; /* header */
    }
    double v[10];
    size_t a = 0;
    int k = 0;
    for (size_t i = 0; i <= line.size() && k < 10; ++i) {
      if (i == line.size() || line[i] == ',') {
        const std::string tok = line.substr(a, i - a);
        char *endp = nullptr;
        if (tok.empty() || std::isspace((unsigned char)tok.front()) || std::isspace((unsigned char)tok.back()))
          return err = "Could not parse float", false;
        v[k] = std::strtod(tok.c_str(), &endp);
        if (!endp || *endp) return err = "Could not parse float", false;
        ++k;
        a = i + 1;
      }
    }
    if (k < 10) return err = "Could not read all ten columns of the camera path", false;
    p.pos.insert(p.pos.end(), v, v + 4);
    p.fwd.insert(p.fwd.end(), v + 4, v + 7);
    p.up.insert(p.up.end(), v + 7, v + 10);
    p.n++;
    if (last) break;
  }
  return p.n > 0 ? true : (err = "empty camera path", false);
}
/* 0 ok, 1 = panic "time outside range", 2 = index out of bounds (the off-by-one) */
int path_camera(const CameraPath &p, double t, double pos[4], double fwd[3], double up[3]) {
  const double min_time = p.pos[0], max_time = p.pos[4 * (p.n - 1)];
  if (t < min_time || t > max_time) return 1;
  double t1 = min_time, t2 = max_time;
  size_t i = 0;
  while (t > p.pos[4 * i]) {
    t1 = p.pos[4 * i];
    t2 = p.pos[4 * (i + 1)];
    i += 1;
  }
  const double frac = (t - t1) / (t2 - t1);
  const size_t i1 = i, i2 = i + 1;
  if (i2 >= p.n) return 2;
  if (!(frac >= 0.0 && frac <= 1.0)) return 1;
  for (int k = 0; k < 4; ++k) pos[k] = p.pos[4 * i1 + k] + frac * (p.pos[4 * i2 + k] - p.pos[4 * i1 + k]);
  for (int k = 0; k < 3; ++k) {
    fwd[k] = p.fwd[3 * i1 + k] + frac * (p.fwd[3 * i2 + k] - p.fwd[3 * i1 + k]);
    up[k] = p.up[3 * i1 + k] + frac * (p.up[3 * i2 + k] - p.up[3 * i1 + k]);
  }
  return 0;
}

}  // namespace

#endif /* CURVIS_CLI_SETTINGS_H */
