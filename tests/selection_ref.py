"""An independent restatement of the selection tool, written from the reference's text (region_growing.cu, selection_utils.cu, correct_mm_operations.cu,
growing_selection.cu:2096-2140): a collections.deque region growing, numpy shift-and-combine dilation / erosion on a boolean [128, 128, 128] array indexed [x, y, z]
with explicit clipping, and the lattice rule of extract_fine_mesh.  Shares no code with the library."""
import collections
import functools

import numpy as np

G = 128
VOL = G ** 3
CASCADES = 5
BITFIELD_BYTES = VOL * CASCADES // 8
CUBE, SPHERE = 0, 1
DILATE, ERODE = 0, 1


def _part(v):
    v = np.asarray(v, np.uint32)
    out = np.zeros_like(v)
    for b in range(7):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def morton(x, y, z):
    return _part(x) | (_part(y) << np.uint32(1)) | (_part(z) << np.uint32(2))


def _compact(m):
    m = np.asarray(m, np.uint32)
    out = np.zeros_like(m)
    for b in range(7):
        out |= ((m >> np.uint32(3 * b)) & np.uint32(1)) << np.uint32(b)
    return out


def invert(pos_idx):
    pos_idx = np.asarray(pos_idx, np.uint32)
    return _compact(pos_idx), _compact(pos_idx >> np.uint32(1)), _compact(pos_idx >> np.uint32(2))


@functools.lru_cache(maxsize=1)
def morton_of_grid():
    """[128, 128, 128] indexed [x, y, z] -> Morton index"""
    a = np.arange(G, dtype=np.uint32)
    return morton(a[:, None, None], a[None, :, None], a[None, None, :])


def upper_cell(cell, target_level):  # get_upper_cell_idx, selection_utils.cu:36-48
    level, pos = int(cell) // VOL, int(cell) % VOL
    x, y, z = (int(v) for v in invert(pos))
    for _ in range(level, target_level):
        x, y, z = x // 2 + G // 4, y // 2 + G // 4, z // 2 + G // 4
    return target_level * VOL + int(morton(x, y, z))


def is_boundary(pos_idx):  # selection_utils.cu:8-13
    x, y, z = (int(v) for v in invert(pos_idx))
    return 0 in (x, y, z) or G - 1 in (x, y, z)


def cell_pos(cells):
    """get_cell_pos (selection_utils.cu:65-68) of each cell at its own level, float32 operation by operation -> [n, 3]"""
    cells = np.asarray(cells, np.uint32)
    level = (cells // np.uint32(VOL)).astype(np.int32)
    xyz = np.stack(invert(cells % np.uint32(VOL)), axis=-1).astype(np.float32)
    f = np.float32
    return (((xyz + f(0.5)) / f(G) - f(0.5)) * np.ldexp(f(1.0), level)[:, None].astype(np.float32) + f(0.5)).astype(np.float32)


def bits_to_grid(bitfield, level):
    """a level of a density-bitfield-layout array -> bool [x, y, z]"""
    bits = np.unpackbits(np.asarray(bitfield, np.uint8)[level * VOL // 8:(level + 1) * VOL // 8], bitorder="little").astype(bool)
    return bits[morton_of_grid()]


def grid_to_bits(grid, level):
    """bool [x, y, z] -> a whole bitfield whose other levels are zero"""
    flat = np.zeros(VOL, np.uint8)
    flat[morton_of_grid().reshape(-1)] = np.asarray(grid, bool).reshape(-1)
    out = np.zeros(BITFIELD_BYTES, np.uint8)
    out[level * VOL // 8:(level + 1) * VOL // 8] = np.packbits(flat, bitorder="little")
    return out


class Growing:
    """RegionGrowing: reset_growing / grow_region (Manual) / upscale_selection"""

    def __init__(self, density_grid, max_cascade):
        self.grid = np.asarray(density_grid, np.float32)
        self.max_cascade = max_cascade
        self.bits = set()              # S as a set of cell indices
        self.cells = []                # L
        self.queue = collections.deque()
        self.level = 0

    def reset(self, seeds, growing_level):
        self.bits, self.cells, self.queue = set(), [], collections.deque()
        for cell in seeds:
            cell = int(cell)
            level = cell // VOL
            if level > growing_level:
                continue
            if level < growing_level:
                cell = upper_cell(cell, growing_level)
            self.queue.append(cell)
            self.cells.append(cell)
        self.level = growing_level

    def upscale(self):
        if self.level == self.max_cascade:
            return
        self.level += 1
        self.cells = [upper_cell(c, self.level) for c in self.cells]
        self.bits = set(self.cells)
        self.queue = collections.deque(upper_cell(c, self.level) for c in self.queue)

    def grow(self, threshold, growing_level, steps):
        if not self.queue:
            return 0
        self.level = growing_level
        popped = 0
        threshold = np.float32(threshold)
        while self.queue and popped < steps:
            cell = self.queue.popleft()
            popped += 1
            level, pos = cell // VOL, cell % VOL
            if cell in self.bits or not self.grid[cell] >= threshold or level != self.level:
                continue
            if is_boundary(pos):
                self.upscale()
                cell = upper_cell(cell, self.level)
                level, pos = cell // VOL, cell % VOL
            x, y, z = (int(v) for v in invert(pos))
            for d, lo in ((-1, True), (1, False)):   # -x, -y, -z, then +x, +y, +z
                for axis in range(3):
                    p = [x, y, z]
                    if (lo and p[axis] > 0) or (not lo and p[axis] < G - 1):
                        p[axis] += d
                        self.queue.append(level * VOL + int(morton(*p)))
            self.cells.append(cell)
            self.bits.add(cell)
        return popped

    def bitfield(self):
        flat = np.zeros(VOL * CASCADES, np.uint8)
        if self.bits:
            flat[np.fromiter(self.bits, np.int64)] = 1
        return np.packbits(flat, bitorder="little")


def _shifted_or(dst, src, d, axis):
    """dst |= src moved by d along axis; what would come from outside the grid is left out (in-grid taps only)"""
    a, b = [slice(None)] * 3, [slice(None)] * 3
    if d > 0:
        a[axis], b[axis] = slice(d, None), slice(None, G - d)
    elif d < 0:
        a[axis], b[axis] = slice(None, G + d), slice(-d, None)
    dst[tuple(a)] |= src[tuple(b)]


def dilate(grid, se_type, r):
    """cell set iff any in-grid tap is set.  Cube: one axis after the other (the same set: with taps outside the grid ignored the cube is a product of three
    clipped intervals).  Sphere: every tap (i, j, k) with i^2 + j^2 + k^2 <= r^2 on its own."""
    grid = np.asarray(grid, bool)
    if se_type == CUBE:
        out = grid
        for axis in range(3):
            nxt = np.zeros_like(out)
            for d in range(-r, r + 1):
                _shifted_or(nxt, out, d, axis)
            out = nxt
        return out
    out = np.zeros_like(grid)
    for i in range(-r, r + 1):
        for j in range(-r, r + 1):
            if i * i + j * j > r * r:
                continue
            plane = np.zeros_like(grid)
            tmp = np.zeros_like(grid)
            _shifted_or(tmp, grid, -i, 0)     # out[x] takes in[x + i]
            _shifted_or(plane, tmp, -j, 1)
            for k in range(-r, r + 1):
                if i * i + j * j + k * k <= r * r:
                    _shifted_or(out, plane, -k, 2)
    return out


def erode(grid, se_type, r):
    """cell set iff no in-grid tap is clear: the clear cells spread like set ones do under dilation, and the outside never contributes"""
    return ~dilate(~np.asarray(grid, bool), se_type, r)


def morph(grid, op, se_type, r):
    return dilate(grid, se_type, r) if op == DILATE else erode(grid, se_type, r)


def brute_cell(grid, x, y, z, op, se_type, r):
    """hit / fit of one cell by the tap loop of CubeSE / SphereSE"""
    for i in range(-r, r + 1):
        for j in range(-r, r + 1):
            for k in range(-r, r + 1):
                if se_type == SPHERE and i * i + j * j + k * k > r * r:
                    continue
                a, b, c = x + i, y + j, z + k
                if not (0 <= a < G and 0 <= b < G and 0 <= c < G):
                    continue
                if op == DILATE and grid[a, b, c]:
                    return True
                if op == ERODE and not grid[a, b, c]:
                    return False
    return op == ERODE


def brute_cell_window(grid, x, y, z, op, se_type, r):
    """the same verdict from the cell's clipped (2r + 1)^3 window at once: every in-grid tap of the element, nothing else"""
    lo = [max(v - r, 0) for v in (x, y, z)]
    hi = [min(v + r, G - 1) for v in (x, y, z)]
    window = grid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    i, j, k = np.ogrid[lo[0] - x:hi[0] - x + 1, lo[1] - y:hi[1] - y + 1, lo[2] - z:hi[2] - z + 1]
    element = np.ones(window.shape, bool) if se_type == CUBE else (i * i + j * j + k * k <= r * r)
    return bool(window[element].any()) if op == DILATE else bool(window[element].all())


def cells_in_loop_order(grid, level):
    """the cell list CorrectMMOperations::dilate / erode leave: x outer, y, z inner"""
    return (np.uint32(level * VOL) + morton_of_grid()[np.asarray(grid, bool)]).astype(np.uint32)   # boolean indexing walks [x, y, z] in C order


def lattice(cells, growing_level):
    """extract_fine_mesh's density_host as [z, y, x] float32 (index x + 128 y + 128^2 z): 1 at every listed cell of the growing level that is not a boundary cell"""
    cells = np.asarray(cells, np.uint32)
    cells = cells[cells // np.uint32(VOL) == growing_level]
    x, y, z = invert(cells % np.uint32(VOL))
    inner = (x > 0) & (y > 0) & (z > 0) & (x < G - 1) & (y < G - 1) & (z < G - 1)
    out = np.zeros((G, G, G), np.float32)
    out[z[inner], y[inner], x[inner]] = 1.0
    return out


def level_box(growing_level):
    s = float(2 ** growing_level)
    return [0.5 - 0.5 * s] * 3, [0.5 + 0.5 * s] * 3


BALL_CENTRE, BALL_RADIUS = (20, 60, 100), 30
LONE_CELLS = ((3, 20, 20), (124, 30, 90), (64, 2, 64), (70, 125, 40), (90, 90, 1), (100, 40, 126))


# ---- the patterns of the morphology tests: name -> bool [x, y, z] ----
def _pattern(name):
    g = np.zeros((G, G, G), bool)
    if name == "full":
        g[:] = True
    elif name == "interior":
        g[70, 41, 93] = True
    elif name == "corners":
        for x in (0, G - 1):
            for y in (0, G - 1):
                for z in (0, G - 1):
                    g[x, y, z] = True
    elif name == "seams":          # runs along x across the word seams 31|32, 63|64, 95|96, and one cell either side of a seam on its own
        g[29:35, 17, 60] = True
        g[62:66, 64, 3] = True
        g[90:101, 127, 77] = True
        g[31, 90, 90] = g[32, 100, 20] = True
    elif name in ("slab_x", "slab_y", "slab_z"):   # a slab on both faces of one axis (122 cells apart: they do not meet at radius <= 10)
        axis = "xyz".index(name[-1])
        idx = [slice(None)] * 3
        for s in (slice(0, 3), slice(G - 3, G)):
            idx[axis] = s
            g[tuple(idx)] = True
    elif name == "random":
        g = np.random.default_rng(20261018).random((G, G, G)) < 0.02
    elif name == "random_inverse":  # 98 % set: what erosion does to a ragged solid (the issue's list has no such pattern; its random field erodes to nothing)
        g = ~_pattern("random")
    elif name in ("ball_noise", "ball_faces"):   # radius-10 elements: a ball of radius 30 round BALL_CENTRE, cut by the x = 0 and z = 127 faces ...
        a = np.arange(G)
        g = (a[:, None, None] - BALL_CENTRE[0]) ** 2 + (a[None, :, None] - BALL_CENTRE[1]) ** 2 + (a[None, None, :] - BALL_CENTRE[2]) ** 2 <= BALL_RADIUS ** 2
        if name == "ball_noise":   # ... in 2 % noise, for erosion: a ragged outside.  (Dilated at radius 10 it is the full grid: of no use there.)
            g |= np.random.default_rng(7).random((G, G, G)) < 0.02
        else:                      # ... and one lone cell near each face, for dilation: most of the grid stays clear
            for x, y, z in LONE_CELLS:
                g[x, y, z] = True
    elif name != "empty":
        raise KeyError(name)
    return g


PATTERNS = ("empty", "full", "interior", "corners", "seams", "slab_x", "slab_y", "slab_z", "random")


@functools.lru_cache(maxsize=None)
def pattern(name):
    g = _pattern(name)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def pattern_morph(name, op, se_type, r):
    """computed once per process and shared, read-only"""
    out = morph(pattern(name), op, se_type, r)
    out.setflags(write=False)
    return out
