"""numpy restatement of compute_verts_normals_packed / compute_faces_normals_packed (src/rep/mesh.jl:589-621, 689-699) and of
their adjoints, in the Float32 operation order include/flux3d_hip.h documents -- the yardstick of the device kernels.

The vertex normals are the reference's CPU semantics: `vertex_normals[:, faces[r, :]] += c_r` is `A[:, I] = A[:, I] + X`, LAST
WRITE WINS for a repeated vertex, so vertex v takes c_r of the last face (in packed face order) whose corner r it is.  The
winners come from an explicit loop in face order (numpy's fancy assignment does not define which duplicate wins).  Every
other step is elementwise Float32 (numpy rounds each operation, no fused multiply-add), and the adjoints' per-vertex sums run
term by term in the documented order.

verts (3, V) float32, faces (3, F) integer 0-based packed ids."""
import numpy as np

EPS = np.float32(1e-6)  # _normalize's eps, T.(1e-6) (src/rep/utils.jl:23-27)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def winners(faces, V):
    """(3, V) int64: w[r, v] = the last face whose corner r is v, -1 if none."""
    w = [[-1] * V for _ in range(3)]
    rows = [list(map(int, faces[r])) for r in range(3)]
    for r in range(3):
        wr, fr = w[r], rows[r]
        for f in range(len(fr)):  # face order: a later face overwrites an earlier one
            wr[fr[f]] = f
    return np.array(w, dtype=np.int64)


def corners(verts, faces):
    """p[k]: (3, F) coordinates of corner k of every face."""
    v = _f32(verts)
    return [v[:, faces[k]] for k in range(3)]


def corner_cross(p, r):
    """c_r = _lg_cross(p[r+1] - p[r], p[r+2] - p[r]) per face (src/rep/utils.jl:4-21), (3, F)."""
    a = p[(r + 1) % 3] - p[r]
    b = p[(r + 2) % 3] - p[r]
    return np.stack([(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])])


def normalize(c):
    """_normalize(c; dims = 1) -> (n, s): c ./ max(s, eps), s = sqrt((x*x + y*y) + z*z); np.maximum keeps a NaN like Julia's max."""
    s = np.sqrt(((c[0] * c[0]) + (c[1] * c[1])) + (c[2] * c[2]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.maximum(s, EPS), s


def raw_verts_normals(verts, faces, w=None):
    V = verts.shape[1]
    w = winners(faces, V) if w is None else w
    p = corners(verts, faces)
    raw = np.zeros((3, V), np.float32)  # the reference's fill!(…, 0.0): +0
    for r in range(3):
        has = w[r] >= 0
        c = corner_cross(p, r)
        raw[:, has] = raw[:, has] + c[:, w[r][has]]
    return raw


def verts_normals(verts, faces, w=None):
    """(3, V) float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return normalize(raw_verts_normals(verts, faces, w))[0]


def faces_normals(verts, faces):
    """(3, F) float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return normalize(corner_cross(corners(verts, faces), 0))[0]


def normalize_bwd(n, s, g):
    """g_raw: (g - n * ((n.x*g.x + n.y*g.y) + n.z*g.z)) / s where s > eps, g / eps elsewhere (NaN s included)."""
    g = _f32(g)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dot = ((n[0] * g[0]) + (n[1] * g[1])) + (n[2] * g[2])
        big = s > EPS
        return np.where(big, (g - (n * dot)) / np.where(big, s, np.float32(1)), g / EPS).astype(np.float32)


def vertex_faces(faces, V):
    """The vertex -> (face, corner) table of fx3d_build_vertex_faces: (rowptr (V+1), face (3F), corner (3F)), entries ascending
    (face, corner) per vertex."""
    vid = np.asarray(faces, np.int64).T.reshape(-1)      # entry f * 3 + t
    order = np.argsort(vid, kind="stable")
    rowptr = np.zeros(V + 1, np.int64)
    np.add.at(rowptr, vid + 1, 1)
    return np.cumsum(rowptr), order // 3, order % 3


def _corner_term(p, r, t, g):
    """Corner t's term of c_r's Jacobian transpose at g: corner r+1 cross(b, g), corner r+2 cross(g, a), corner r their
    negated sum (a = p[r+1] - p[r], b = p[r+2] - p[r]); arrays over items."""
    a = p[(r + 1) % 3] - p[r]
    b = p[(r + 2) % 3] - p[r]
    da = np.stack([(b[1] * g[2]) - (b[2] * g[1]), (b[2] * g[0]) - (b[0] * g[2]), (b[0] * g[1]) - (b[1] * g[0])])
    db = np.stack([(g[1] * a[2]) - (g[2] * a[1]), (g[2] * a[0]) - (g[0] * a[2]), (g[0] * a[1]) - (g[1] * a[0])])
    return np.where(t == r, -(da + db), np.where(t == (r + 1) % 3, da, db))


def _gather(verts, faces, graw_of_role, roles_valid, base):
    """g[u] = base[u] (or +0) + the terms of u's entries (f, t) ascending, roles r = 0, 1, 2 in order, one at a time."""
    V = verts.shape[1]
    rowptr, ef, et = vertex_faces(faces, V)
    p = corners(verts, faces)
    deg = np.diff(rowptr)
    eu = np.repeat(np.arange(V), deg)                     # the vertex of every entry (CSR order)
    terms = np.zeros((3, len(ef), 3), np.float32)
    valid = np.zeros((len(ef), 3), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            ok = roles_valid(r, ef)
            valid[:, r] = ok
            pe = [q[:, ef] for q in p]
            terms[:, :, r] = _corner_term(pe, r, et, graw_of_role(r, ef))
    items_u = np.repeat(eu, 3)[valid.reshape(-1)]
    items_terms = terms.reshape(3, -1)[:, valid.reshape(-1)]
    # position of every item within its vertex's ordered list, then one vectorised step per position
    start = np.searchsorted(items_u, np.arange(V))
    rank = np.arange(len(items_u)) - start[items_u]
    acc = np.zeros((3, V), np.float32) if base is None else _f32(base).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == k
            u = items_u[sel]                               # distinct vertices: plain assignment is well defined
            acc[:, u] = acc[:, u] + items_terms[:, sel]
    return acc


def verts_normals_bwd(verts, faces, gout, base=None):
    """Adjoint of verts_normals w.r.t. verts: (3, V) float32; `base`: the accumulate form's starting gradient."""
    verts = _f32(verts)
    V = verts.shape[1]
    w = winners(faces, V)
    with np.errstate(invalid="ignore", over="ignore"):
        n, s = normalize(raw_verts_normals(verts, faces, w))
    graw = normalize_bwd(n, s, gout)
    F = faces.shape[1]
    win = np.zeros((3, F), bool)                           # (f, r) is the winner of its owner faces[r, f]
    for r in range(3):
        win[r] = w[r][faces[r]] == np.arange(F)
    return _gather(verts, faces, lambda r, ef: graw[:, faces[r][ef]], lambda r, ef: win[r][ef], base)


def faces_normals_bwd(verts, faces, gout, base=None):
    """Adjoint of faces_normals w.r.t. verts: (3, V) float32."""
    verts = _f32(verts)
    with np.errstate(invalid="ignore", over="ignore"):
        n, s = normalize(corner_cross(corners(verts, faces), 0))
    graw = normalize_bwd(n, s, gout)
    return _gather(verts, faces, lambda r, ef: graw[:, ef], lambda r, ef: np.full(len(ef), r == 0), base)


def sheet(nx, ny, seed=0):
    """A jittered (nx x ny)-cell sheet, 0-based faces: (nx+1)(ny+1) vertices, 2 nx ny triangles (the shape of the mesh timings)."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 0) + rng.uniform(-0.3, 0.3, (3, gx.size))
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).ravel()
    f = np.concatenate([np.stack([a, a + ny + 1, a + ny + 2]), np.stack([a, a + ny + 2, a + 1])], 1)
    return np.asfortranarray(v.astype(np.float32)), np.asfortranarray(f.astype(np.int64))
