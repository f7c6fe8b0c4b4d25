"""Golden vectors of Visualizer.overlay_instances, draw_dataset_dict and draw_instance_predictions as they were BEFORE overlay_instances
went through amp_render_instances: the SHA-256 and the shape of every image of tests/render_cases.py golden_renders(), written to
tests/golden/render_vectors.json.  Run on the commit whose ampis_amd/utils/visualizer.py still draws every instance with full-image NumPy
passes and one PIL round trip per label; tests/test_render.py holds the later code to these hashes, so that nothing a caller sees changes.

    python tests/golden/make_render_vectors.py        # needs the built library (the RLE codec rasterises the polygons)

Only hashes and shapes are stored; the inputs are the committed fixtures read through tests/seg_perf_data.py and synthetic arrays."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import render_cases as rc  # noqa: E402


def main():
    import inspect
    from ampis_amd.utils.visualizer import Visualizer
    assert "render_instances" not in inspect.getsource(Visualizer), "run this on the Visualizer that still draws instance by instance"
    out = {name: {"shape": list(img.shape), "sha256": hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()}
           for name, img in rc.golden_renders().items()}
    with open(os.path.join(ROOT, "tests", "golden", "render_vectors.json"), "w") as f:
        json.dump({"made_by": "tests/golden/make_render_vectors.py", "images": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
