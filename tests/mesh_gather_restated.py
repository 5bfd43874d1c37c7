"""chisel_hip_gather_meshes restated in numpy: the marker colours of FillMarkerTopicWithMeshes in float32, one
operation per line, and the gather as a concatenation of per-mesh arrays with its table.  The GPU tests compare the library against
these and against GetMesh; nothing here touches the library."""
import numpy as np

F = np.float32


def marker_rgba(normals, light0, light1, diffuse, ambient):
    """(V, 3) float32 normals -> (V, 4) float32: r = g = b = fminf((s0 + s1) + ambient, 1), a = 1, with
    s_k = fmaxf((n.x l_k.x + n.y l_k.y) + n.z l_k.z, 0) diffuse; a NaN normal gives s_k = 0 (fmaxf returns its other argument)"""
    n = np.asarray(normals, F).reshape(-1, 3)
    l0, l1 = np.asarray(light0, F), np.asarray(light1, F)
    diffuse, ambient = F(diffuse), F(ambient)
    s = []
    with np.errstate(invalid="ignore", over="ignore"):
        for l in (l0, l1):
            px = n[:, 0] * l[0]
            py = n[:, 1] * l[1]
            pz = n[:, 2] * l[2]
            d = px + py
            d = d + pz
            m = np.fmax(d, F(0.0))
            s.append(m * diffuse)
        c = s[0] + s[1]
        c = c + ambient
        c = np.fmin(c, F(1.0))
    out = np.empty((len(n), 4), F)
    out[:, 0] = out[:, 1] = out[:, 2] = c
    out[:, 3] = F(1.0)
    assert out.dtype == F and c.dtype == F
    return out


def color_rgba(colors):
    """a map with colour: the mesh colour of the vertex, a = 1"""
    c = np.asarray(colors, F).reshape(-1, 3)
    return np.concatenate([c, np.ones((len(c), 1), F)], axis=1)


def gather(meshes, lights=None):
    """meshes: a list of dicts as Chisel.GetMesh returns them, in the selection's order -> the dict GatherMeshes returns for it
    (without "ids"): every array the concatenation of the meshes' own, rgba from the colours where the meshes have them, else from
    the normals and `lights`; table row i = (first vertex, vertices, first grid, grids), zeros for an empty mesh"""
    cat = lambda key, w: (np.concatenate([np.asarray(m[key], F).reshape(-1, w) for m in meshes], axis=0) if meshes else np.zeros((0, w), F))
    has_color = bool(meshes) and all(m.get("colors") is not None for m in meshes)
    res = {"vertices": cat("vertices", 3), "normals": cat("normals", 3), "colors": cat("colors", 3) if has_color else None, "grids": cat("grids", 3)}
    if lights is not None:
        res["rgba"] = color_rgba(res["colors"]) if has_color else marker_rgba(res["normals"], lights["light0"], lights["light1"], lights["diffuse"], lights["ambient"])
    sizes = np.array([[len(m["vertices"]), len(m["grids"])] for m in meshes], np.int64).reshape(-1, 2)
    first = np.cumsum(sizes, axis=0) - sizes
    table = np.stack([first[:, 0], sizes[:, 0], first[:, 1], sizes[:, 1]], axis=1) if len(meshes) else np.zeros((0, 4), np.int64)
    table[(sizes == 0).all(axis=1)] = 0
    res["table"] = table
    return res
