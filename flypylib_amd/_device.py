"""The torch side of the device stages (batchgen.DeviceBatches, mine.py, labels.py): torch or
a message, the resident-tensor test and the device a `device=` argument names.  Each stage
passes its own phrase, so every message still says which stage it came from."""


def require_torch(what, hint):
    """torch, or RuntimeError('<what> torch (...); <hint>')"""
    try:
        import torch
    except Exception as e:      # noqa: BLE001
        raise RuntimeError('%s torch (%s: %s); %s' % (what, type(e).__name__, e, hint))
    return torch


def is_device_tensor(a):
    return hasattr(a, 'is_cuda') and hasattr(a, 'data_ptr') and bool(a.is_cuda)


def torch_device(device, what, load):
    """torch.device of `device` (an int, or True for the runtime's default device).  `load()`
    - the stage's load_library - runs first: a library that is not built is reported before
    a GPU that is not there."""
    import torch
    load()
    if device is True:
        from . import runtime
        device = runtime.default_device()
    device = int(device)
    if not torch.cuda.is_available() or device >= torch.cuda.device_count():
        raise RuntimeError('%s on cuda:%d: torch sees %d GPUs'
                           % (what, device, torch.cuda.device_count() if torch.cuda.is_available() else 0))
    return torch.device('cuda', device)
