"""Serial rendering of the reference's VTK file -- TEST INFRASTRUCTURE ONLY. tests/test_vtk.py holds
the writer against it, tests/test_gpu_output.py the driver's whole files."""
import numpy as np

TRIAX_HEADER = b"SCALARS TRIAX_STRESS float 1\nLOOKUP_TABLE default\n"   # the file's last block


def serial_vtk(coordmat, elementmat, flag, disp, velo, ns, nn, ne, nm, nt):
    """Line-by-line restatement of write_vtk's output (v2/HAKAI_j.jl:3564-3712) with Python's
    printf-style "%1.6e" (the reference's @printf format) and its |x| < 1e-16 flush (:3530-3558)."""
    def f16(x):
        return 0.0 if abs(x) < 1e-16 else x

    def e(x):  # Julia's @printf spells non-finite values NaN / Inf / -Inf
        if not np.isfinite(x):
            return "NaN" if np.isnan(x) else ("Inf" if x > 0 else "-Inf")
        return "%1.6e" % x

    nN, nE = coordmat.size // 3, flag.size
    out = ["# vtk DataFile Version 2.0\nTest\nASCII\nDATASET UNSTRUCTURED_GRID\n", f"POINTS {nN} float\n"]
    X = coordmat.reshape(-1, 3)
    out += [f"{e(a)} {e(b)} {e(c)}\n" for a, b, c in X]
    draw = int(flag.sum())
    out.append(f"CELLS {draw} {draw * 9}\n")
    em = elementmat.reshape(-1, 8)
    out += ["8 " + " ".join(str(int(v) - 1) for v in em[i]) + "\n" for i in range(nE) if flag[i] == 1]
    out.append(f"CELL_TYPES {draw}\n")
    out += ["12\n"] * draw
    out.append(f"POINT_DATA {nN}\nVECTORS DISPLACEMENT float\n")
    out += [f"{e(f16(a))} {e(f16(b))} {e(f16(c))}\n" for a, b, c in disp.reshape(-1, 3)]

    def scal(name, vals):
        out.append(f"SCALARS {name} float 1\nLOOKUP_TABLE default\n")
        out.extend(e(f16(v)) + "\n" for v in vals)

    for c, n in enumerate(("Vx", "Vy", "Vz")):
        scal(n, velo.reshape(-1, 3)[:, c])
    for c, n in enumerate(("E11", "E22", "E33", "E12", "E23", "E13")):
        scal(n, nn.reshape(-1, 6)[:, c])
    scal("EQ_PSTRAIN", ne)
    for c, n in enumerate(("S11", "S22", "S33", "S12", "S23", "S13")):
        scal(n, ns.reshape(-1, 6)[:, c])
    scal("MISES_STRESS", nm)
    scal("TRIAX_STRESS", nt)
    return "".join(out).encode()
