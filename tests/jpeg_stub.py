"""A stand-in for the device call of ``hawq_amd.jpeg.decode_jpeg_batch``, for the tests of its bookkeeping that run without a GPU."""
import torch


def stub_launch(monkeypatch, models, entry, statuses=None):
    """``jpeg._launch`` replaced by Python models writing into the caller's host tensor.  ``models``: {"base" | "prog": record -> uint8
    [H, W, 3]}, one per kind of record the test lets through; ``statuses``: {kind: {position among the records of that call: status}},
    such an image is left as it is; ``entry(kind, records, out, sync)``: what the returned list of calls receives per call."""
    from hawq_amd import jpeg
    calls = []

    def launch(records, out_offsets, out, dev, events=None, sync=None, info=None):
        kind = "prog" if isinstance(records[0], jpeg.JpegProgRecord) else "base"
        status = torch.zeros(len(records), dtype=torch.int32)
        for k, (r, off) in enumerate(zip(records, out_offsets)):
            if statuses and k in statuses.get(kind, {}):
                status[k] = statuses[kind][k]
                continue   # a failed image leaves garbage
            rgb = models[kind](r)
            out[off:off + rgb.size] = torch.from_numpy(rgb.reshape(-1))
        calls.append(entry(kind, records, out, sync))
        return status

    monkeypatch.setattr(jpeg, "_launch", launch)
    return calls
