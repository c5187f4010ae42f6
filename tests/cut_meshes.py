"""The cut meshes off the centred circle on the square mesh: one catalogue for tests/test_cut_meshes_cpu.py (which asserts what makes
it a valid judge) and tests/test_gpu_cut_general.py (which judges the product's cutHHO side on it).

Every mesh breaks the symmetry of the N x N unit square with the centred circle: Nx != Ny, a box that is not the unit square (so
hx != hy, or min_x / min_y != 0), a circle off the centre.  An `Nx` written for `Ny`, an i / j swap, a dropped `min_x`, `hx` for `hy`
or a prefix count that needs mirror-symmetric cut cells changes the result on at least one of them.

  name  Nx x Ny  box                      level set
  A     14 x 10  [0, 1.4] x [0, 1]        circle r 0.33 at (0.66, 0.53)          square cells, Nx != Ny
  At    10 x 14  [0, 1] x [0, 1.4]        circle r 0.33 at (0.53, 0.66)          A with x and y exchanged
  B     15 x 11  [-0.5, 1] x [0.2, 1.3]   circle r 0.36 at (0.21, 0.77)          shifted box, both origins non-zero
  C     13 x 8   [0, 1.3] x [0, 0.8]      circle r 0.27 at (0.61, 0.43)
  E     9 x 5    [2, 3.5] x [-1, -0.25]   line y = -0.58                         far from the origin, hx != hy
  G     12 x 9   unit square              circle r 0.36 at (0.48, 0.53)          hx / hy = 0.75
  D     12 x 7   unit square              circle r 0.35 at (0.5, 0.5)            hx / hy = 0.583: four cut cells with a negative-side
                                                                                 area fraction of 0.097 whose k = 2 systems are not SPD

CLEAN: the meshes on which binary128 (oracle/cut_truth.c) and the oracle factor every cut cell at k = 0, 1, 2.  D_REFUSED: the cells
of D binary128 refuses at k = 2 (one-sided system on the negative side, and the interface system)."""
import functools
from collections import namedtuple

Mesh = namedtuple("Mesh", "name Nx Ny lo hi radius center line_y")

CATALOGUE = {m.name: m for m in (
    Mesh("A", 14, 10, (0.0, 0.0), (1.4, 1.0), 0.33, (0.66, 0.53), None),
    Mesh("At", 10, 14, (0.0, 0.0), (1.0, 1.4), 0.33, (0.53, 0.66), None),
    Mesh("B", 15, 11, (-0.5, 0.2), (1.0, 1.3), 0.36, (0.21, 0.77), None),
    Mesh("C", 13, 8, (0.0, 0.0), (1.3, 0.8), 0.27, (0.61, 0.43), None),
    Mesh("E", 9, 5, (2.0, -1.0), (3.5, -0.25), 0.0, (0.0, 0.0), -0.58),
    Mesh("G", 12, 9, (0.0, 0.0), (1.0, 1.0), 0.36, (0.48, 0.53), None),
    Mesh("D", 12, 7, (0.0, 0.0), (1.0, 1.0), 0.35, (0.5, 0.5), None),
)}
CLEAN = ("A", "At", "B", "C", "E", "G")
CIRCLES = tuple(n for n, m in CATALOGUE.items() if m.line_y is None)
A_REFSTEPS = (0, 1, 4, 6)               # A at 2-4, 4-8, 32-64 and 128-256 interface points per cell
D_REFUSED = (25, 34, 49, 58)
KAPPAS = ((1.0, 1.0), (1.0, 7.5))
MAX_CELLS = 165
COND_GATE = 1.9e9                       # the worst 1-norm condition number test_gpu_cuthho.judge_cut_cells' 1e-12 gate covers


def kwargs(name):
    """what BatchAssembler.cut_preprocess and oracle_lib.CutMesh take after N (= Nx) and refsteps"""
    m = CATALOGUE[name]
    kw = dict(Ny=m.Ny, lo=m.lo, hi=m.hi)
    if m.line_y is None:
        kw.update(radius=m.radius, center=m.center)
    else:
        kw.update(line_y=m.line_y)
    return kw


@functools.lru_cache(maxsize=None)
def oracle_mesh(name, refsteps=4, agglomeration=False):
    """the oracle's preprocessed mesh, once per (mesh, level, branch); never modified"""
    import oracle_lib as o
    return o.CutMesh(CATALOGUE[name].Nx, refsteps=refsteps, agglomeration=agglomeration, **kwargs(name))


def preprocess(asm, name, refsteps=4, rows=None, agglomeration=False):
    """the product's preprocessing of the same mesh -> number of cut cells"""
    return asm.cut_preprocess(CATALOGUE[name].Nx, refsteps=refsteps, rows=rows, agglomeration=agglomeration, **kwargs(name))


def cut_cells(msh):
    import numpy as np
    import oracle_lib as o
    return np.nonzero(msh.cell_loc == o.CUT_ON_INTERFACE)[0]


def face_direction(msh):
    """per face: 0 horizontal (along x), 1 vertical (along y)"""
    import numpy as np
    p = msh.points[msh.faces.astype(np.int64)]
    d = np.abs(p[:, 1] - p[:, 0])
    return (d[:, 1] > d[:, 0]).astype(np.int8)
