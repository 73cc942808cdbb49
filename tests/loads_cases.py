"""Decks with external loads for the reader and driver tests -- TEST INFRASTRUCTURE ONLY.

write_loads_deck writes a Model with tests/inp_writer.py and adds what that writer does not know:
assembly-level sets and surfaces (before *End Assembly), *Amplitude tables (after it) and the load
blocks of the step (before *End Step), each given as text."""
import numpy as np

from inp_writer import write_inp


def write_loads_deck(path, m, assembly="", amplitudes="", step=""):
    write_inp(path, m)
    text = open(path).read()
    assert text.count("*End Assembly\n") == 1 and text.count("*End Step\n") == 1
    text = text.replace("*End Assembly\n", assembly + "*End Assembly\n" + amplitudes)
    text = text.replace("*End Step\n", step + "*End Step\n")
    with open(path, "w") as f:
        f.write(text)
    return path


def elset(name, elements, instance="P1-1"):
    """An assembly element set the reader resolves (the 'internal' list form)."""
    ids = [int(e) for e in elements]
    lines = "".join(", ".join(str(x) for x in ids[a:a + 16]) + "\n" for a in range(0, len(ids), 16))
    return f"*Elset, elset={name}, internal, instance={instance}\n{lines}"


def nset(name, nodes, instance="P1-1"):
    ids = [int(n) for n in nodes]
    lines = "".join(", ".join(str(x) for x in ids[a:a + 16]) + "\n" for a in range(0, len(ids), 16))
    return f"*Nset, nset={name}, instance={instance}\n{lines}"


def amplitude(name, t, v):
    return f"*Amplitude, name={name}\n" + ", ".join(f"{float(a)!r}, {float(b)!r}" for a, b in zip(t, v)) + "\n"


def bar_end_elements(nx, ny, nz, top=True):
    """1-based elements of the z = 0 or z = L layer of a mesh.bar_model (ids x-fastest, then y, z)."""
    k = nz - 1 if top else 0
    return np.arange(k * nx * ny, (k + 1) * nx * ny) + 1
