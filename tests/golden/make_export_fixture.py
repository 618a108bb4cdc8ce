"""Generates tests/golden/export_live_rig.npz: scripts/export_reference_gums.py run on a LIVE GUMStereo of the imported
reference (the distorted rig of make_fixtures.py, the object a user's pickle holds).

Runs ONLY where the reference tree is importable (see make_fixtures.py); the test that reads the fixture needs neither
the reference nor its placeholder modules.
    PYTHONPATH=/path/to/vo_single_camera_sos PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_export_fixture.py

The live object is wrapped in a proxy that records every attribute the exporter reads (leaf values only: numbers,
strings, arrays), so the fixture holds
  attr:<path>  -- each value the exporter read, e.g. attr:top_model.precalib_params.k1
  doc          -- the JSON document the exporter wrote for the live object
  {top,bot}_lut_{x,y}_sha256 / _nan / _shape -- digests of the reference's own full Panorama LUTs (float64, NaN
                  entries zeroed for hashing, their positions kept as a mask)
  {top,bot}_lut_rows / _lut_{x,y} -- a few full rows of the same LUTs, to show where a digest mismatch lies.
No reference source text is stored.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "export_live_rig.npz")
LEAF = (np.ndarray, np.generic, float, int, bool, str, tuple, list, type(None))


class Recorder(object):
    """Attribute access on `obj` through this proxy is logged into `log` as {dotted path: value} for leaf values;
    non-leaf values come back wrapped in another Recorder.  A missing attribute raises AttributeError as the object
    would, so getattr(..., default) in the exporter takes the same branch."""

    def __init__(self, obj, path, log):
        object.__setattr__(self, "_obj", obj)
        object.__setattr__(self, "_path", path)
        object.__setattr__(self, "_log", log)

    def __getattr__(self, name):
        v = getattr(self._obj, name)
        path = self._path + name
        if isinstance(v, LEAF):
            self._log[path] = v
            return v
        return Recorder(v, path + ".", self._log)


def lut_digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    nan = np.isnan(a)
    return hashlib.sha256(np.where(nan, 0.0, a).tobytes()).hexdigest(), nan


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "scripts"))
    import make_fixtures as mf
    import export_reference_gums as exp
    gum, pano, cm, ccv, pet = mf.import_reference()
    gs, top, bot = mf.build_gums_distorted(gum, pano)
    log = {}
    doc = exp.gums_to_sosvo_json(Recorder(gs, "", log))
    assert doc == exp.gums_to_sosvo_json(gs), "the proxy changed what the exporter sees"
    out = {"doc": np.array(json.dumps(doc, sort_keys=True))}
    for path, v in log.items():
        out["attr:" + path] = np.asarray(v)
    for name, m in (("top", top), ("bot", bot)):
        rows = np.linspace(0, m.panorama.world2cam_LUT_map_x.shape[0] - 1, 7).round().astype(np.int64)
        out[name + "_lut_rows"] = rows
        for ax in ("x", "y"):
            lut = np.asarray(getattr(m.panorama, "world2cam_LUT_map_" + ax), dtype=np.float64)
            digest, nan = lut_digest(lut)
            out["%s_lut_%s_sha256" % (name, ax)] = np.array(digest)
            out["%s_lut_%s_nan" % (name, ax)] = np.packbits(nan.ravel())
            out["%s_lut_%s_shape" % (name, ax)] = np.array(lut.shape, dtype=np.int64)
            out["%s_lut_%s" % (name, ax)] = lut[rows]
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "(%d attributes read by the exporter)" % len(log))


if __name__ == "__main__":
    main()
