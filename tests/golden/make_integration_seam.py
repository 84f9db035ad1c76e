"""Generate tests/golden/integration_seam.json: what the REFERENCE's own u2_arch.py / u2llama.py build for the arguments of
tests/test_integration_seam.py, recorded so that the test runs without the reference tree.

    python tests/golden/make_integration_seam.py <reference checkout>

Recorded: the state dict of the model the unswapped reference builds (`initialize_vision_modules`, u2_arch.py:29-78), key
for key and shape for shape; the class names of the three modules it builds; the two properties the reference reads off
them (`vision_tower.hidden_size`, u2_arch.py:68; `mm_projector.proj_out_num`, train_stage1.py:369); and the messages of the
ValueErrors its builders raise for an unknown tower / projector name.  MONAI is absent offline: vit.py:19-20 imports the
two MONAI blocks from the stub of make_golden.py (parameter names = MONAI's)."""
import importlib
import importlib.util
import json
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from test_integration_seam import LLAMA, MODEL_ARGS  # noqa: E402

OUT = HERE / "integration_seam.json"


def main(reference):
    sys.path.insert(0, str(Path(reference).resolve()))
    spec = importlib.util.spec_from_file_location("_u2_make_golden", HERE / "make_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mk.install_monai_stub()
    llama = importlib.import_module("src.model.language_model.u2llama")

    def construct(args):
        torch.manual_seed(0)
        m = llama.u2LlamaForCausalLM(llama.u2Config(**LLAMA))
        m.get_model().initialize_vision_modules(NS(**args))
        return m

    m = construct(MODEL_ARGS)
    mm = m.get_model()
    errors = {}
    for key, args in (("vision_tower", dict(MODEL_ARGS, vision_tower="resnet")),
                      ("mm_projector", dict(MODEL_ARGS, mm_projector_type="qformer"))):
        try:
            construct(args)
        except ValueError as e:
            errors[key] = str(e)
    assert set(errors) == {"vision_tower", "mm_projector"}, errors
    rec = {"model_args": MODEL_ARGS, "llama": LLAMA,
           "state_dict": {k: list(v.shape) for k, v in m.state_dict().items()},
           "classes": {n: type(getattr(mm, n)).__name__ for n in ("vision_tower", "mm_projector", "u2tokenizer")},
           "vision_hidden_size": mm.vision_tower.hidden_size, "mm_hidden_size": mm.config.mm_hidden_size,
           "proj_out_num": mm.mm_projector.proj_out_num, "errors": errors}
    OUT.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(f"wrote {OUT} ({len(rec['state_dict'])} tensors)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
