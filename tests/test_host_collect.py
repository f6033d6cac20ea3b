"""Runs, by its name, right before tests/test_host_logic.py.

Owners of captured graphs die in reference cycles (a module, its capture cache, the captured closure) and stay uncollected until
Python's next FULL collection, which in a long process is rare.  utils/graphed.py deliberately forces no collection when a recording
opens, so an explicit ``gc.collect()`` inside a recording parks every such owner the earlier GPU tests left behind — and
test_host_logic.py counts what is parked.  Whether a full collection happened to run in between depended on how much the suite
allocates, that is, on every test that is ever added.  Here the collection runs where it is harmless: outside any recording."""
import gc

from paddlexde_amd.utils import graphed


def test_dead_owners_of_captured_graphs_are_collected_outside_a_recording():
    assert graphed.recordings_open() == 0
    gc.collect()
    assert not graphed._DEFERRED  # (nothing is parked with no recording open: the owners were released as they were collected)
