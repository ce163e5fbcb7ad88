"""Writes tests/golden/flat_update_host_digest.json: sha256 digests of the node and order tables the HOST builder (rt_tables.h build_tables +
build_flat_bvh, through tests/flatbvh's fb_scene_tables) makes for the worlds of tests/test_flat_update_cpu.py.  Recorded from the builder
as it was before flat_entry_box moved into rt_flat_build.h; run it again only when the builder is MEANT to build other bytes.
    python tests/golden/make_flat_update_digest.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the repository root on the path)
import test_flat_update_cpu as T  # noqa: E402

if __name__ == "__main__":
    abi = conftest.graft.load_package().abi
    out = T.host_build_digests(abi)
    with open(os.path.join(HERE, "flat_update_host_digest.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
