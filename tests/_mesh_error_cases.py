"""The hand-made cases of the point-to-mesh tests (tests/test_mesh_error_host.py on the CPU, tests/test_gpu_mesh_error.py on the
device): one triangle with a point in each of its regions, and the degenerate triangles."""
import numpy as np

# one triangle in the plane z = 1, a right angle at A; exactly representable, so the analytic values are exact
A, B, C = np.array([0.0, 0.0, 1.0]), np.array([4.0, 0.0, 1.0]), np.array([0.0, 3.0, 1.0])
# (point, squared distance): the seven regions above the plane, then on the plane, on an edge, at a corner
REGIONS = [
    ((1.0, 1.0, 3.0), 4.0),                                              # face
    ((2.0, -2.0, 2.0), 5.0),                                             # edge AB
    ((-1.0, 1.0, 3.0), 5.0),                                             # edge CA
    ((5.0, 5.5, 3.0), 29.0),                                             # edge BC: its midpoint (2, 1.5) plus (3, 4), 2 above
    ((-1.0, -2.0, 0.0), 6.0),                                            # corner A
    ((6.0, -1.0, 2.0), 6.0),                                             # corner B
    ((-1.0, 5.0, 1.0), 5.0),                                             # corner C
    ((1.0, 1.0, 1.0), 0.0),                                              # on the plane, inside
    ((5.0, -1.0, 1.0), 2.0),                                             # on the plane, outside: corner B
    ((2.0, 0.0, 1.0), 0.0),                                              # on edge AB
    ((2.0, 1.5, 1.0), 0.0),                                              # on edge BC
    ((0.0, 3.0, 1.0), 0.0),                                              # at corner C
    ((2.0, 0.0, -2.0), 9.0),                                             # above edge AB: face and edge agree
    ((0.0, 0.0, 5.0), 16.0),                                             # above corner A
]
U, V_, M_ = np.array([1.0, 2.0, 3.0]), np.array([5.0, 4.0, 7.0]), np.array([3.0, 3.0, 5.0])       # M_ the midpoint of U V_
DEGENERATE = [("two equal", (U, U, V_)), ("two equal", (U, V_, V_)), ("two equal", (V_, U, V_)), ("all equal", (U, U, U)),
              ("collinear", (U, M_, V_)), ("collinear", (M_, V_, U))]
DEGENERATE_POINTS = [(0.0, 0.0, 0.0), (3.0, 3.0, 5.0), (9.0, 1.0, 2.5), (1.0, 2.0, 3.0), (-4.0, 8.0, 0.25), (4.0, 3.5, 6.0)]
