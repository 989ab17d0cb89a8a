"""An independent float64 reading of the subdivision rules (psdr_jit_amd/subdiv.py states them): a per-face Python loop over dictionaries that shares
no code with the package.  reference_level() returns the rows of S as {column: float64 weight} dictionaries, the fine faces and the edge counts;
matrix() turns rows into a scipy CSR matrix in float64.  Also the small meshes the CPU and GPU tests share."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "examples", "data", "mesh", "bunny_low.obj")
CBOX = os.path.join(ROOT, "examples", "data", "cbox")

TETRAHEDRON = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
BOWTIE = [[0, 1, 2], [0, 3, 4]]                 # two triangles that share only vertex 0
BOOK = [[0, 1, 2], [0, 1, 3], [0, 1, 4]]        # three faces on the edge (0, 1)


def grid(m):
    """(m - 1)^2 squares, two triangles each, over m x m vertices"""
    faces = []
    for i in range(m - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, i * m + j + 1, (i + 1) * m + j, (i + 1) * m + j + 1
            faces += [[a, b, d], [a, d, c]]
    return faces, m * m


def fan(k):
    """k triangles round hub 0, rim 1 .. k, and vertex k + 1 that no face uses"""
    return [[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], k + 2


def load_obj(path):
    """(faces, n, positions, face_uv, uvs) of a triangulated OBJ file; face_uv / uvs None without `vt`"""
    v, vt, f, ft = [], [], [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(s) for s in t[1:4]])
            elif t[0] == "vt":
                vt.append([float(s) for s in t[1:3]])
            elif t[0] == "f":
                corners = [s.split("/") for s in t[1:]]
                for k in range(1, len(corners) - 1):
                    tri = (corners[0], corners[k], corners[k + 1])
                    f.append([int(c[0]) - 1 for c in tri])
                    if len(tri[0]) > 1 and tri[0][1]:
                        ft.append([int(c[1]) - 1 for c in tri])
    has_uv = bool(vt) and len(ft) == len(f)
    return f, len(v), np.array(v, np.float64), (ft if has_uv else None), (np.array(vt, np.float64) if has_uv else None)


def reference_level(faces, n, scheme):
    """(rows, fine_faces, E, sharp): rows[i] = {column: weight} of fine vertex i, in float64"""
    opposite = {}                                    # undirected edge -> the third vertex of every face at it
    for a, b, c in faces:
        for p, q, o in ((a, b, c), (b, c, a), (c, a, b)):
            opposite.setdefault((min(p, q), max(p, q)), []).append(o)
    edges = sorted(opposite)
    number = {e: i for i, e in enumerate(edges)}
    E = len(edges)
    rows = [dict() for _ in range(n + E)]
    ends = [[] for _ in range(n)]                    # per vertex: (the other end, is the edge sharp)
    sharp = 0
    for e in edges:
        is_sharp = len(opposite[e]) != 2
        sharp += is_sharp
        ends[e[0]].append((e[1], is_sharp))
        ends[e[1]].append((e[0], is_sharp))
        row = rows[n + number[e]]
        if scheme == "linear" or is_sharp:
            row[e[0]] = 0.5
            row[e[1]] = 0.5
        else:
            row[e[0]] = 3.0 / 8.0
            row[e[1]] = 3.0 / 8.0
            for o in opposite[e]:
                row[o] = row.get(o, 0.0) + 1.0 / 8.0
    for v in range(n):
        d = len(ends[v])
        s = sum(1 for _, sh in ends[v] if sh)
        if scheme == "linear" or d == 0:
            rows[v][v] = 1.0
        elif s == 0:
            beta = 3.0 / 16.0 if d == 3 else 3.0 / (8.0 * d)
            rows[v][v] = 1.0 - d * beta
            for o, _ in ends[v]:
                rows[v][o] = beta
        elif s == 2:
            rows[v][v] = 3.0 / 4.0
            for o, sh in ends[v]:
                if sh:
                    rows[v][o] = 1.0 / 8.0
        else:
            rows[v][v] = 1.0
    fine = []
    for a, b, c in faces:
        ab, bc, ca = (n + number[(min(p, q), max(p, q))] for p, q in ((a, b), (b, c), (c, a)))
        fine += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
    return rows, fine, E, sharp


def matrix(rows, n_in):
    """the rows as a scipy CSR matrix in float64, columns ascending"""
    import scipy.sparse as sp
    row_begin, col, val = [0], [], []
    for r in rows:
        for j in sorted(r):
            col.append(j)
            val.append(r[j])
        row_begin.append(len(col))
    return sp.csr_matrix((np.array(val, np.float64), np.array(col, np.int64), np.array(row_begin, np.int64)), shape=(len(rows), n_in))


_LEVELS = {}


def reference_chain(key, faces, n, scheme, levels):
    """[(S64, fine_faces, E, sharp)] per level, level l + 1 from level l's fine faces; computed once per `key` and shared (do not modify)"""
    k = (key, scheme, levels)
    if k not in _LEVELS:
        out, f = [], [list(t) for t in np.asarray(faces).tolist()]
        for _ in range(levels):
            rows, fine, E, sharp = reference_level(f, n, scheme)
            out.append((matrix(rows, n), fine, E, sharp))
            f, n = fine, n + E
        _LEVELS[k] = out
    return _LEVELS[k]
