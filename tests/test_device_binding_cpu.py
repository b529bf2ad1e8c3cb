"""device_binding.DeviceBinding without a GPU: Engine and BatchEngine share one buffer check, one stream ordering and one binder;
what is not a buffer is refused, each thing for its own reason; and everything a caller gave is validated before anything is
allocated -- on a machine without a GPU allocating on "cuda" raises something that is no ValueError, so a ValueError proves the
order (with a GPU the same calls raise the same ValueError)."""
import pytest
import torch

CAP = 16


@pytest.fixture(scope="module", params=["Engine", "BatchEngine"])
def handle(sb, request):
    h = getattr(sb, request.param).__new__(getattr(sb, request.param))
    h._h, h.device, h.max_particles, h.max_beams, h._ext_stream = None, 0, CAP, CAP, None
    h.n_scenes = 2
    return h


class OnDevice(torch.Tensor):
    """A host tensor that says it is on cuda:0, so that the checks behind the device check can be reached without a GPU
    (nothing here is ever handed to the library)."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def on_device(*shape, dtype=torch.int32):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)


def test_both_classes_share_one_implementation(sb):
    binding = sb.engine.DeviceBinding
    assert sb.batch.DeviceBinding is binding and issubclass(sb.Engine, binding) and issubclass(sb.BatchEngine, binding)
    for name in ("_device_buffer", "_ordered", "_bind"):
        assert getattr(sb.Engine, name) is getattr(sb.BatchEngine, name) is getattr(binding, name), name
        assert name not in vars(sb.Engine) and name not in vars(sb.BatchEngine), name
    assert not hasattr(sb.Engine, "_streams")
    assert (sb.Engine._owner, sb.BatchEngine._owner) == ("engine", "batch")


# what is refused, and the words of the refusal that tell the reasons apart; 64 bytes of int32 are asked for
REFUSED = [("a string", lambda: "no", "not str"),
           ("a bool", lambda: True, "not bool"),
           ("a CPU tensor", lambda: torch.zeros(CAP, dtype=torch.int32), "is on cpu"),
           ("a wrong dtype", lambda: on_device(CAP, dtype=torch.float32), "int32 tensor is needed"),
           ("not contiguous", lambda: on_device(CAP, 2)[:, 0], "contiguous"),
           ("one element too small", lambda: on_device(CAP - 1), "at least 64 bytes is needed, this one has 60")]


@pytest.mark.parametrize("what, make, words", REFUSED, ids=[r[0] for r in REFUSED])
def test_what_is_not_a_buffer_is_refused(handle, what, make, words):
    with pytest.raises(ValueError, match=words):
        handle._device_buffer("call: x", make(), "int32", CAP * 4)
    with pytest.raises(ValueError, match="call: x: .*" + words):
        handle._bind("call", [("x", make(), True, (CAP,), "int32")])
    with pytest.raises(ValueError, match=words):     # also where it is not wanted, and behind an output that would be allocated
        handle._bind("call", [("made", None, True, (CAP,), "int32"), ("x", make(), False, (CAP,), "int32")])


def test_what_is_a_buffer_passes(handle):
    assert handle._device_buffer("x", 4096, "int32", 64) == (4096, False)
    t = on_device(CAP)
    assert handle._device_buffer("x", t, ("float32", "int32"), 64) == (t.data_ptr(), True)
    assert handle._device_buffer("x", on_device(8, dtype=torch.float64), None, 64)[1] is True      # None: any dtype
    assert handle._owner in str(pytest.raises(ValueError, handle._device_buffer, "x", torch.zeros(CAP), None, 4).value)


def test_bind_views_a_given_tensor_and_sizes_eight_byte_words(handle):
    """A flat, oversized tensor comes back as a view of the shape over the same storage, one that has the shape as the same
    object, a pointer as it is; an int64 entry needs 8 bytes a word."""
    flat, exact = on_device(3 * CAP + 5), on_device(CAP, 2)
    (a, b, c, d), (pa, pb, pc, pd), tensors = handle._bind("call", [
        ("a", flat, True, (CAP, 3), "int32"), ("b", exact, True, (CAP, 2), "int32"), ("c", 4096, True, (CAP,), "int64"),
        ("d", on_device(CAP), False, (CAP,), "int32")])
    assert tuple(a.shape) == (CAP, 3) and a.data_ptr() == flat.data_ptr() == pa and a.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    assert b is exact and pb == exact.data_ptr() and (c, pc) == (4096, 4096) and (d, pd) == (None, None) and tensors is True
    assert handle._bind("call", [("c", 4096, True, (CAP,), "int64")])[2] is False
    with pytest.raises(ValueError, match="at least 128 bytes"):
        handle._bind("call", [("c", on_device(CAP - 1, dtype=torch.int64), True, (CAP,), "int64")])
    handle._bind("call", [("c", on_device(CAP, dtype=torch.int64), True, (CAP,), "int64")])


def bad():
    return torch.zeros(4 * CAP, dtype=torch.int64)     # on the host: refused, whatever is asked for


ORDER = {"bodies": lambda e: e.bodies(counts=bad()),                      # labels would be allocated first
         "graph": lambda e: e.graph(adjacency=True, counts=bad()),         # ends, row_ptr and nbr
         "contacts": lambda e: e.contacts(pairs=8, labels=bad()),          # touch, counts and pairs
         "body_summary": lambda e: e.body_summary(rows=4, labels=bad())}   # out


@pytest.mark.parametrize("name", sorted(ORDER))
def test_engine_validates_before_it_allocates(sb, name):
    eng = sb.Engine.__new__(sb.Engine)
    eng._h, eng.device, eng.max_particles, eng.max_beams, eng._ext_stream = None, 0, CAP, CAP, None
    with pytest.raises(ValueError, match="%s: (counts|labels): the tensor is on cpu" % name):
        ORDER[name](eng)


def test_engine_refuses_a_bool_where_it_has_no_meaning(sb):
    eng = sb.Engine.__new__(sb.Engine)
    eng._h, eng.device, eng.max_particles, eng.max_beams, eng._ext_stream = None, 0, CAP, CAP, None
    for call in (lambda: eng.summary(out=True), lambda: eng.summary(out=False), lambda: eng.contacts(pairs=4, out=True),
                 lambda: eng.body_summary(labels=False), lambda: eng.write_particles_device(True)):
        with pytest.raises(ValueError, match="not bool"):
            call()


def test_a_bad_rows_pairs_or_adjacency_still_comes_first(sb):
    """... before the buffers are looked at: the message is the argument's, though a buffer of the same call is bad too."""
    eng = sb.Engine.__new__(sb.Engine)
    eng._h, eng.device, eng.max_particles, eng.max_beams, eng._ext_stream = None, 0, CAP, CAP, None
    for rows in (0, CAP + 1, True, 2.0, None):
        with pytest.raises(ValueError, match="rows is"):
            eng.body_summary(rows=rows, out="no")
    for pairs in (-1, True, 2.5, "8"):
        with pytest.raises(ValueError, match="pairs is"):
            eng.contacts(pairs=pairs, touch="no")
    with pytest.raises(ValueError, match="out needs a pair list"):
        eng.contacts(pairs=0, out=on_device(8), touch="no")
    with pytest.raises(ValueError, match="nbr without row_ptr"):
        eng.graph(adjacency=(False, True), ends="no")
    with pytest.raises(ValueError, match="unpack"):
        eng.graph(adjacency=(True, True, True), ends="no")
