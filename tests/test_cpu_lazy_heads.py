"""detector.LazyHeads without a GPU: the dict a sparse-heads run returns as res["heads"] completes its maps on the first access of any
form, once, and every form of access sees the completed values (a fake completer stands in for the deferred dense launches)."""
import pytest

import h3d_amd  # noqa: F401
from h3d_amd.detector import LazyHeads


def _make():
    maps = {"hm": [1.0], "wh": [None], "pose": [None]}      # one-element lists stand in for the tensors: completion fills them in place
    calls = []

    def completer():
        calls.append(1)
        maps["wh"][0], maps["pose"][0] = 2.0, 3.0

    return LazyHeads(maps, completer), calls


ACCESS = {
    "getitem": lambda h: h["wh"][0],
    "get": lambda h: h.get("wh")[0],
    "items": lambda h: dict(h.items())["wh"][0],
    "values": lambda h: list(h.values())[1][0],
    "iter": lambda h: [k for k in h] and dict.__getitem__(h, "wh")[0],
    "contains": lambda h: ("wh" in h) and dict.__getitem__(h, "wh")[0],
    "dict": lambda h: dict(h)["wh"][0],
    "copy": lambda h: h.copy()["wh"][0],
}


@pytest.mark.parametrize("form", sorted(ACCESS))
def test_every_access_form_completes_once_and_sees_complete_values(form):
    heads, calls = _make()
    assert not calls and not heads.complete
    assert ACCESS[form](heads) == 2.0, form
    assert calls == [1] and heads.complete
    for other in sorted(ACCESS):                    # idempotent: no access form completes a second time
        assert ACCESS[other](heads) == 2.0
    assert calls == [1]


def test_dict_and_items_hold_every_completed_map_in_head_order():
    heads, calls = _make()
    d = dict(heads)
    assert list(d) == ["hm", "wh", "pose"] and [v[0] for v in d.values()] == [1.0, 2.0, 3.0] and calls == [1]
    heads2, calls2 = _make()
    assert [(k, v[0]) for k, v in heads2.items()] == [("hm", 1.0), ("wh", 2.0), ("pose", 3.0)] and calls2 == [1]


def test_keys_and_len_do_not_complete_and_rearm_makes_the_next_access_complete_again():
    heads, calls = _make()
    assert list(heads.keys()) == ["hm", "wh", "pose"] and len(heads) == 3 and not calls
    heads["hm"]
    assert calls == [1]
    again = []
    heads.rearm(lambda: again.append(1))            # a graph replay rewrote the sparse maps: the next access runs the new completer
    assert not heads.complete
    heads.get("wh")
    heads["pose"]
    assert again == [1] and calls == [1]


def test_a_failing_completer_leaves_the_dict_incomplete():
    def boom():
        raise RuntimeError("launch failed")
    heads = LazyHeads({"hm": [0.0]}, boom)
    with pytest.raises(RuntimeError, match="launch failed"):
        heads["hm"]
    assert not heads.complete
