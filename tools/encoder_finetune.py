"""Fine-tuning of the heads TOGETHER WITH every decoder layer and every scene-encoder layer
(CtRLSim.set_trainable("heads+decoder+encoder")) over a frozen map encoder and frozen embeddings: tools/head_finetune.py's loop — logged
scenes -> dataset -> windows -> training_step_ctx / optimizer_step on one generated batch — printing the loss per step.

    python tools/encoder_finetune.py [steps=20] [B=32]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_finetune  # noqa: E402

if __name__ == "__main__":
    head_finetune.main("heads+decoder+encoder")
