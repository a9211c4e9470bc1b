"""The scenes of tests/test_gpu_step_scale.py, as data: tests/test_step_scale_host.py walks the same lists and asserts, from the composed
reference alone and without a GPU, that every scene holds the ray classes its case is meant to cover."""
import step_scale_ref as SR

EQUIRECTANGULAR = 1


def _case(kind, pose, S, **kw):
    c = dict(kind=kind, pose=pose, S=S, **kw)
    c["id"] = "-".join([kind, pose, str(S)] + ["%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in sorted(kw.items())])
    return c


# debug dump and plain fused frame: three metrics, four poses, both scales (S = 870 makes kappa inexact), a cap low enough that capped
# and escaped rays coexist, one ragged frame
DUMP = [
    _case("ellis", "facing", 1024), _case("ellis", "tilted", 870), _case("ellis", "negative", 1024), _case("ellis", "inside", 870),
    _case("interstellar", "facing", 870), _case("interstellar", "tilted", 1024), _case("interstellar", "negative", 870),
    _case("interstellar", "inside", 1024),
    _case("flat", "facing", 1024), _case("flat", "tilted", 870),
    _case("ellis", "inside", 1024, cap=260, capped=True),
    _case("interstellar", "tilted", 870, res=SR.RES_RAGGED),
]
BATCH = [_case("ellis", pose, 1024) for pose in ("facing", "tilted", "negative")]          # three poses in one launch (all in DUMP's scenes)
BAND = _case("ellis", "facing", 1024)
SUPERSAMPLED = _case("ellis", "facing", 1024)                                              # the fine frame of a 20 x 12 camera at N = 2
FILTERED = _case("ellis", "facing", 1024, skies="fine")
PROJECTED = _case("interstellar", "facing", 1024, projection=EQUIRECTANGULAR, res=(32, 16))
ALL_THREE = _case("ellis", "tilted", 870, projection=EQUIRECTANGULAR, res=(32, 16), skies="fine")   # the fine frame of a 16 x 8 camera at N = 2
BRUTE = DUMP + [FILTERED, PROJECTED, ALL_THREE]

ANGLE = [dict(_case(kind, "facing", S), renderer=r, id="%s-%s-%d" % (r, kind, S))
         for r in ("direct", "efficient") for kind, S in (("ellis", 1024), ("interstellar", 870))]
