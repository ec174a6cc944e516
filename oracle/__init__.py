"""oracle/ -- CPU restatement of the reference's ICP + PointFusion hot path.

TEST INFRASTRUCTURE ONLY.  Nothing under ``gradslam_amd/`` may import this package; the only
legal importers are ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of
``bench.py`` -- and there only as the checker / the timed CPU baseline, never as the product.

What it is: a functional restatement, in fp32 torch-CPU ops plus one plain-C file for the
K=1 nearest-neighbour search, of the algorithm in the reference's

* ``gradslam/structures/rgbdimages.py:643-762``  (vertex / normal maps)        -> maps.py
* ``gradslam/odometry/icputils.py:22-669``        (ICP, gradICP, downsampling)   -> icp.py
* ``gradslam/slam/fusionutils.py:16-789``         (PointFusion map update)       -> fusion.py
* ``gradslam/slam/icpslam.py:99-264``, ``slam/pointfusion.py:107-112`` (frame loop) -> slam.py
* ``gradslam/geometry/{se3utils,projutils,geometryutils}.py`` pieces the path calls -> geometry.py
* one step of ``odometry/icputils.py:310-367, :479-545`` from a device trace row, and the loops in float64 with
  autograd, for the step and reverse-pass tests                                     -> icp_step.py

Each function cites the reference file:line it follows.  It uses the same torch ops in the same
order wherever rounding or an integer decision depends on it, so that on CPU it reproduces the
reference's numbers (checked by tests/test_oracle_golden.py against tests/golden/*.npz, which
were produced by importing the unmodified reference -- see tools/gen_golden.py).

Parity pinning status
* everything except the nearest-neighbour search: pinned by golden vectors generated from the
  reference itself plus the reference's own fixtures (tests/golden/msrd_b2s3.npz) and
  known-answer tests.
* K=1 nearest neighbour (3rd-party ``chamferdist==1.0.0``, source absent from the reference
  tree): per-point indices are PARITY-UNPINNED by the reference; the contract restated here
  (squared L2, x->y->z accumulation, strict ``<`` so the lowest index wins) is pinned only through
  the reference's converged-pose tests (tests/odometry/test_icp.py:14-53, test_gradicp.py:14-60).
"""
