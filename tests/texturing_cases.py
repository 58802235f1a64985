"""Cases shared by tests/test_texturing_cpu.py (through the numpy restatement) and tests/test_texturing_gpu.py (through the kernels): small enough for seconds,
with the selection labels worked out by hand here, not taken from either implementation."""
import functools

import numpy as np

H, W = 48, 64
K = np.array([[32.0, 0.0, 32.0], [0.0, 32.0, 24.0], [0.0, 0.0, 1.0]])  # fx = fy = 2^5: a point (X, Y, 1) lands on (32 X + 32, 32 Y + 24) exactly
IDENTITY = np.eye(4)


def ramp_frame():
    """An integer affine ramp of the pixel coordinates per channel, inside 0 .. 255."""
    row, col = np.mgrid[0:H, 0:W]
    return np.stack([2 * col + row + 3, col + 3 * row + 10, 255 - 3 * col - row], axis=-1).astype(np.uint8)


def ramp(sx, sy):
    """The same ramp at a real screen point (what an exact bilinear fetch returns inside the image)."""
    return np.array([2 * sx + sy + 3, sx + 3 * sy + 10, 255 - 3 * sx - sy], np.float64)


def quad(sx0, sx1, sy0, sy1, z=1.0, colour=(10, 200, 90)):
    """Two faces on the plane z = const of the identity camera whose corners project to (sx0 | sx1, sy0 | sy1): the even face (v00, v10, v01), the odd face
    (v11, v01, v10) -- so block-local texel (x, y) maps affinely to the screen for either."""
    X = lambda sx: (sx - 32.0) / 32.0 * z
    Y = lambda sy: (sy - 24.0) / 32.0 * z
    vertices = np.array([[X(sx0), Y(sy0), z], [X(sx1), Y(sy0), z], [X(sx0), Y(sy1), z], [X(sx1), Y(sy1), z]], np.float64)
    return dict(vertices=vertices, faces=np.array([[0, 1, 2], [3, 2, 1]], np.int32), vertex_colors=np.tile(np.array(colour, np.uint8), (4, 1)))


def join(*meshes):
    base, V, F, C = 0, [], [], []
    for m in meshes:
        V.append(m["vertices"]), F.append(m["faces"] + base), C.append(m["vertex_colors"])
        base += len(m["vertices"])
    return dict(vertices=np.concatenate(V), faces=np.concatenate(F).astype(np.int32), vertex_colors=np.concatenate(C))


# the known-answer quad: corners at (30.5 | 33.5, 22.25 | 25.25); with S - 5 a power of two every sample point is exactly representable
QUAD_CORNERS = (30.5, 33.5, 22.25, 25.25)


def behind_pose(cx=0.25, cz=4.0):
    """World-to-camera of a camera at (cx, 0, cz) looking down -z (a half turn about y): cam = (cx - x, y, cz - z)."""
    pose = np.diag([-1.0, 1.0, -1.0, 1.0])
    pose[:3, 3] = [cx, 0.0, cz]
    return pose


def two_quads(gap):
    """A front quad at z = 1 (screen 24 .. 40 x 16 .. 32 in view 0) and a smaller back quad at z = 1 + gap right behind its middle.  View 0 is the identity
    camera; view 1 looks from behind the pair (there is no back-face test), where the back quad is the nearer one and both project smaller than in view 0.
    The front quad's depth plane in view 0 is exactly 1.0f (q_e = w_e / 1, den = A), and a back vertex has z_k = 1 + gap exactly (identity pose, last row of K
    0 0 1), so view 0 keeps the back faces iff 1 + gap <= 1.0 + tolerance in float64."""
    z = np.float64(1.0) + np.float64(gap)
    back = dict(vertices=np.array([[-0.125, -0.125, z], [0.125, -0.125, z], [-0.125, 0.125, z], [0.125, 0.125, z]], np.float64),
                faces=np.array([[0, 1, 2], [3, 2, 1]], np.int32), vertex_colors=np.tile(np.array([200, 30, 30], np.uint8), (4, 1)))
    return join(quad(24.0, 40.0, 16.0, 32.0), back), np.stack([IDENTITY, behind_pose()])


TOLERANCE = 0.05
# (gap, labels by hand): hidden from view 0 by far more than the tolerance -> view 1; exactly at the tolerance -> a candidate in both, view 0's area is the
# larger (depth 1.05 against 2.95); one float64 step above -> hidden from view 0 again
TWO_QUAD_LABELS = [(1.0, [0, 0, 1, 1]), (TOLERANCE, [0, 0, 0, 0]), (float(np.nextafter(np.float64(1.0) + np.float64(TOLERANCE), 2.0) - 1.0), [0, 0, 1, 1])]


def frames_for(n, seed=0):
    rng = np.random.default_rng(100 + seed)
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def random_poses(n, seed):
    """Small random rotations and shifts about the identity camera."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(200 + seed)
    poses = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        poses[k, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.15, 0.15, 3)).as_matrix()
        poses[k, :3, 3] = rng.uniform(-0.2, 0.2, 3)
    return poses


def soup(nf, seed):
    """nf random triangles a few pixels across in front of the identity camera, a few behind it or off screen."""
    rng = np.random.default_rng(300 + seed + nf)
    centre = np.stack([rng.uniform(-1.2, 1.2, nf), rng.uniform(-0.9, 0.9, nf), rng.uniform(0.8, 3.0, nf)], axis=1)
    centre[rng.random(nf) < 0.05, 2] = -0.5
    vertices = (centre[:, None, :] + rng.uniform(-0.12, 0.12, (nf, 3, 3))).reshape(-1, 3)
    return dict(vertices=vertices, faces=np.arange(3 * nf, dtype=np.int32).reshape(nf, 3), vertex_colors=rng.integers(0, 256, (3 * nf, 3), dtype=np.uint8))


def masks_for(n, seed):
    rng = np.random.default_rng(400 + seed)
    masks = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        i, j = rng.integers(0, H - 16), rng.integers(0, W - 16)
        masks[k, i:i + 16, j:j + 16] = 1 + k
    return masks


SOUP_FACES, SOUP_CELLS, SOUP_VIEWS = (1, 2, 3, 255, 256, 257, 513), (6, 9, 16), (1, 3)


def soup_case(nf, cell, n, with_masks):
    seed = nf * 7 + cell * 3 + n
    return dict(mesh=soup(nf, seed), frames=frames_for(n, seed), poses=random_poses(n, seed), masks=masks_for(n, seed) if with_masks else None, cell=cell)


@functools.lru_cache(maxsize=None)
def room():
    """The synthetic room fused into a 32^3 volume by the oracle: (mesh dict, sequence, world-to-camera poses)."""
    import oracle
    from hive_amd import synthetic
    seq = synthetic.make_sequence(num_frames=3, height=H, width=W, yaw_step_deg=25.0)
    volume = oracle.TSDFVolume(synthetic.room_bounds(), 0.16)  # 5.12 m / 0.16 m = 32 voxels a side
    for i in range(3):
        volume.integrate(seq["color"][i], seq["depth"][i], seq["K"], seq["poses"][i])
    vertices, faces, _, colors = volume.get_mesh()
    mesh = dict(vertices=np.asarray(vertices, np.float64), faces=np.asarray(faces, np.int32), vertex_colors=np.asarray(colors, np.uint8))
    return mesh, seq, np.linalg.inv(seq["poses"])


def reverse_labels(views, n):
    """The labels of a run whose views were passed in reverse order, in the original numbering."""
    views = np.asarray(views)
    return np.where(views < 0, -1, n - 1 - views).astype(np.int32)
