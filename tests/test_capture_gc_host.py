"""not gpu: `mingpt._no_gc_while_capturing` -- dead cycles are collected before a stream capture and the automatic collector is paused
while one lasts (a collection inside a capture finalises device objects on the capturing thread, which aborts inside the HIP runtime;
DESIGN.md section 4.17)."""
import gc
import threading
import weakref


def test_collector_is_paused_while_capturing_and_restored():
    from ccvs_amd.models.skip_vid_generator.models.mingpt import _no_gc_while_capturing

    class Node:
        pass

    a, b = Node(), Node()
    a.other, b.other = b, a                                              # a dead cycle once the names go
    dead = weakref.ref(a)
    del a, b
    assert gc.isenabled() and dead() is not None
    entered, release = threading.Event(), threading.Event()

    def other_capture():
        with _no_gc_while_capturing():
            entered.set()
            release.wait(30)

    with _no_gc_while_capturing():
        assert dead() is None and not gc.isenabled()                     # collected on entry, paused inside
        thread = threading.Thread(target=other_capture)
        thread.start()
        assert entered.wait(30)
    assert not gc.isenabled()                                            # the other thread's capture still lasts
    release.set()
    thread.join()
    assert gc.isenabled()
    gc.disable()                                                         # a caller that runs without the collector keeps it off
    try:
        with _no_gc_while_capturing():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
