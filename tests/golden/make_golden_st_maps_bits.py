"""Records the bytes of the structure-tensor maps -> tests/golden/st_maps_bits.json.

Needs the GPU.  Per case (a route of st.st_maps at one shape) three calls: want=OUTPUTS with normalize on, the same with normalize off,
and gt=None with want=("Sx", "Fx"); per call the SHA-256 of the bytes of every output.  The kernels are bit-reproducible from run to
run, so a replay is compared for equality.  Record it from a checkout of the commit whose bits are to be preserved:

    python tests/golden/make_golden_st_maps_bits.py

tests/test_st_maps_bits_gpu.py replays it against the tree under test.
"""
import hashlib
import json
import os
import sys
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "st_maps_bits.json")

SEED = 21
# (sigma, rho), forced down the general route: the two tile builds, the general route at radii (4, 8) and at its bound (8, 20), and
# the first tile build's pair through the separable passes
ROUTES = OrderedDict([("tile (2,8)", ((0.5, 2.0), False)), ("tile (4,10)", ((1.0, 2.5), False)), ("general (4,8)", ((1.0, 2.0), False)),
                      ("general (8,20)", ((2.0, 5.0), False)), ("(2,8) forced general", ((0.5, 2.0), True))])
# partial tiles on both axes with W no multiple of 4; smaller than every halo; exactly one tile
SHAPES = ((2, 33, 31), (1, 5, 3), (2, 32, 32))


def images(b, h, w):
    """-> (sr, gt) on the CPU: gt uniform in [0, 1], sr = (gt + 0.1 * randn).clamp(0, 1)."""
    import torch
    g = torch.Generator().manual_seed(SEED)
    gt = torch.rand(b, 3, h, w, generator=g)
    return (gt + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1), gt


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(route, shape):
    """-> {call: {output: sha256}} of the three calls of one case."""
    import torch
    from srganst import loss as L
    from srganst import st
    (sigma, rho), force = ROUTES[route]
    sr, gt = (t.cuda() for t in images(*shape))
    saved = L.ST_FORCE_GENERAL
    try:
        L.ST_FORCE_GENERAL = force
        calls = OrderedDict([("normalize", st.st_maps(sr, gt, sigma, rho, True, want=st.OUTPUTS)),
                             ("normalize=False", st.st_maps(sr, gt, sigma, rho, False, want=st.OUTPUTS)),
                             ("gt=None", st.st_maps(sr, None, sigma, rho, want=("Sx", "Fx")))])
        torch.cuda.synchronize()
    finally:
        L.ST_FORCE_GENERAL = saved
    return OrderedDict((call, OrderedDict((k, _sha(v)) for k, v in outs.items())) for call, outs in calls.items())


def cases():
    """name -> function() -> the record of one case."""
    return OrderedDict((f"{route} at {list(shape)}", lambda route=route, shape=shape: run(route, shape)) for route in ROUTES for shape in SHAPES)


def main():
    recs = OrderedDict((name, fn()) for name, fn in cases().items())
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:                 # one line per case: a changed case is one changed line
        f.write('{"seed": %d, "cases": {\n' % SEED)
        f.write(",\n".join(f"{json.dumps(name)}: {json.dumps(r, separators=(',', ':'))}" for name, r in recs.items()))
        f.write("\n}}\n")
    print(len(recs), "cases")


if __name__ == "__main__":
    main()
