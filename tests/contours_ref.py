"""The dense reference of amp_mask_contours: the boundary rings of ONE decoded mask, straight from the definition.  It shares no code with the
run-based implementation and knows no run lists: every unit boundary edge is collected from pixel neighbours -- a pixel's top side runs left
to right, its right side downwards, its bottom side right to left, its left side upwards, so the one lies on the right hand --, and the edges
are walked vertex by vertex; where a vertex has two outgoing edges (a saddle) the walk turns left for connectivity 2 and right for 1.  A ring
keeps the vertices where the direction changes, starts at its smallest corner by (x, y), and the rings are ordered by that corner."""
import numpy as np

DX = (1, 0, -1, 0)                                # directions east, south, west, north: clockwise on screen, y down
DY = (0, 1, 0, -1)


def boundary_edges(mask):
    """{(x, y): [directions of the boundary edges that start there]} of a bool [h, w] mask"""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    out = {}
    rr, cc = np.nonzero(m)
    for r, c in zip(rr.tolist(), cc.tolist()):
        y, x = r - 1, c - 1
        if not m[r - 1, c]:
            out.setdefault((x, y), []).append(0)                    # top side, heading east
        if not m[r, c + 1]:
            out.setdefault((x + 1, y), []).append(1)                # right side, heading south
        if not m[r + 1, c]:
            out.setdefault((x + 1, y + 1), []).append(2)            # bottom side, heading west
        if not m[r, c - 1]:
            out.setdefault((x, y + 1), []).append(3)                # left side, heading north
    return out


def crack_perimeter(mask):
    """the number of unit pixel sides between a one and a zero, the outside of the image counting as zero"""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    return int((m[1:, :] != m[:-1, :]).sum() + (m[:, 1:] != m[:, :-1]).sum())


def rings(mask, connectivity):
    """the rings of a bool [h, w] mask as a list of {'xy': int32 [k, 2], 'area2': int, 'length': int}, in canonical form and order"""
    assert connectivity in (1, 2)
    edges = boundary_edges(mask)
    seen = set()
    found = []
    for start in sorted(edges):
        for d0 in edges[start]:
            if (start, d0) in seen:
                continue
            pts, (x, y), d, length = [], start, d0, 0
            while True:
                seen.add(((x, y), d))
                x, y, length = x + DX[d], y + DY[d], length + 1
                out = edges[(x, y)]
                if len(out) == 1:
                    nd = out[0]
                else:                                                # a saddle: both turns are open, never straight on
                    nd = (d + 3) % 4 if connectivity == 2 else (d + 1) % 4
                    assert sorted(out) == sorted(((d + 3) % 4, (d + 1) % 4))
                if nd != d:
                    pts.append((x, y))
                d = nd
                if (x, y) == start and d == d0:
                    break
            k = pts.index(min(pts))
            pts = pts[k:] + pts[:k]
            nxt = pts[1:] + pts[:1]
            area2 = sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(pts, nxt))
            assert length == sum(abs(a[0] - b[0]) + abs(a[1] - b[1]) for a, b in zip(pts, nxt))
            found.append({"xy": np.array(pts, dtype=np.int32).reshape(-1, 2), "area2": int(area2), "length": int(length)})
    assert len(seen) == sum(len(v) for v in edges.values())
    found.sort(key=lambda r: (int(r["xy"][0, 0]), int(r["xy"][0, 1])))
    return found
