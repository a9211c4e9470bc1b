"""The scenes of tests/test_gpu_integrator.py, as data: tests/test_integrator_host.py walks the same lists and asserts, from the composed
reference alone and without a GPU, that every scene holds the ray classes its case is meant to cover.  The scenes are those of
tests/gpu_step_scale_cases.py (R = 30, the four poses and three metrics of step_scale_ref, index skies) under integrator = 1, at
delta = 0.1 (integrator_ref.DELTA) but for one case at 0.05, with step_scale in {0, 1024, 870}."""
import step_scale_ref as SR

EQUIRECTANGULAR = 1


def _case(kind, pose, S, **kw):
    c = dict(kind=kind, pose=pose, S=S, **kw)
    c["id"] = "-".join([kind, pose, str(S)] + ["%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in sorted(kw.items())])
    return c


# debug dump and plain fused frame: three metrics, four poses, fixed steps and both scales (S = 870 makes kappa inexact), a cap low
# enough that capped and escaped rays coexist, one ragged frame, one frame at the reference's delta
DUMP = [
    _case("ellis", "facing", 1024), _case("ellis", "tilted", 870), _case("ellis", "negative", 0), _case("ellis", "inside", 870),
    _case("interstellar", "facing", 870), _case("interstellar", "tilted", 0), _case("interstellar", "negative", 870),
    _case("interstellar", "inside", 1024),
    _case("flat", "facing", 1024), _case("flat", "tilted", 0),
    _case("ellis", "inside", 1024, cap=130, capped=True),
    _case("interstellar", "tilted", 870, res=SR.RES_RAGGED),
    _case("ellis", "facing", 1024, delta=0.05),
]
BATCH = [_case("ellis", "facing", 1024), _case("ellis", "tilted", 1024), _case("ellis", "negative", 1024)]   # three poses in one launch
BAND = _case("ellis", "facing", 1024)
SUPERSAMPLED = _case("ellis", "facing", 1024)                                              # the fine frame of a 20 x 12 camera at N = 2
FILTERED = _case("ellis", "facing", 0, skies="fine")
PROJECTED = _case("interstellar", "facing", 1024, projection=EQUIRECTANGULAR, res=(32, 16))
ALL_THREE = _case("ellis", "tilted", 870, projection=EQUIRECTANGULAR, res=(32, 16), skies="fine")   # the fine frame of a 16 x 8 camera at N = 2
BRUTE = DUMP + BATCH[1:] + [FILTERED, PROJECTED, ALL_THREE]

ANGLE = [dict(_case(kind, "facing", S), renderer=r, id="%s-%s-%d" % (r, kind, S))
         for r in ("direct", "efficient") for kind, S in (("ellis", 1024), ("interstellar", 870), ("ellis", 0))]
