"""Writes tests/golden/keras_writer_h5py.json: for every case of tests/test_keras_h5.py::test_writer_round_trip_and_real_h5py, the
sha256 of the file ubdvss_amd.keras_h5_writer writes and what the REAL libhdf5 / h5py reads from that file (layer and weight names,
shapes, value sums, attributes, model_config).  The test then checks that the writer still emits exactly those bytes, so the suite
needs no h5py.  Re-run after a change to the writer, with this project's interpreter, naming one that has h5py (not a dependency):
    python tests/golden/make_keras_writer_golden.py /path/to/python-with-h5py
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ubdvss_amd import keras_h5_writer  # noqa: E402
from ubdvss_amd.net import weight_shapes  # noqa: E402

H5PY_CHECK = r"""
import sys, json, h5py, numpy as np
path, want_model = sys.argv[1], sys.argv[2] == "1"
f = h5py.File(path, "r")
out = {"root_attrs": sorted(f.attrs.keys())}
g = f["model_weights"] if want_model else f
out["layer_names"] = [n.decode() for n in g.attrs["layer_names"]]
out["backend"] = g.attrs["backend"].decode(); out["keras_version"] = g.attrs["keras_version"].decode()
names, sums, shapes = [], [], []
for n in out["layer_names"]:
    for w in g[n].attrs["weight_names"]:
        d = g[n][w.decode()]
        assert d.dtype == np.float32
        names.append(w.decode()); shapes.append(list(d.shape)); sums.append(float(np.asarray(d[()], np.float64).sum()))
out["weight_names"], out["shapes"], out["sums"] = names, shapes, sums
if want_model:
    cfg = json.loads(f.attrs["model_config"].decode())
    out["classes"] = [l["class_name"] for l in cfg["config"]["layers"]]
    out["cfg_names"] = [l["name"] for l in cfg["config"]["layers"]]
    out["model_class"] = cfg["class_name"]; out["outputs"] = cfg["config"]["output_layers"]
print(json.dumps(out))
"""


def main(h5py_python):
    spec = importlib.util.spec_from_file_location("test_keras_h5", os.path.join(os.path.dirname(HERE), "test_keras_h5.py"))
    tk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tk)                     # the test's cases and weights: one source for both
    versions = subprocess.run([h5py_python, "-c", "import h5py; print(h5py.__version__, h5py.version.hdf5_version)"],
                              check=True, capture_output=True, text=True).stdout.split()
    out = {"h5py": versions[0], "hdf5": versions[1], "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for c_in, n_cls, fml, whole in tk.WRITER_CASES:
            path = os.path.join(tmp, "out.h5")
            keras_h5_writer.write_keras_model(path, tk._expected(200 + c_in + n_cls, weight_shapes(c_in, n_cls)), c_in, n_cls, fml, whole)
            with open(path, "rb") as f:
                sha = hashlib.sha256(f.read()).hexdigest()
            r = subprocess.run([h5py_python, "-c", H5PY_CHECK, path, "1" if whole else "0"], check=True, capture_output=True, text=True)
            out["cases"][f"{c_in},{n_cls},{int(fml)},{int(whole)}"] = {"sha256": sha, "h5py": json.loads(r.stdout.strip().splitlines()[-1])}
    with open(os.path.join(HERE, "keras_writer_h5py.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
