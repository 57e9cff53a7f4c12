"""Fine-tuning of the heads TOGETHER WITH the whole last decoder layer — its feed-forward block, its cross-attention sublayer and its
causal self-attention sublayer (CtRLSim.set_trainable("heads+last_layer")) — over an otherwise frozen trunk: tools/head_finetune.py's loop — logged scenes -> dataset ->
windows -> training_step_ctx / optimizer_step on one generated batch — printing the loss per step.

    python tools/last_layer_finetune.py [steps=20] [B=32]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_finetune  # noqa: E402

if __name__ == "__main__":
    head_finetune.main("heads+last_layer")
