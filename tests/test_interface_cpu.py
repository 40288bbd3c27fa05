"""CPU: the signatures of the trainer and the harness that callers, tools and saved scripts depend on, and the package's public
names, spelled out: a rearrangement of the host code must leave every one as it is."""
import inspect

P, K = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY"
NO = inspect.Parameter.empty

FIT = [("clip_dir", P, NO), ("out_path", P, NO), ("epochs", P, 80), ("batch_size", P, 16), ("patience", P, 12), ("max_t", P, 90),
       ("lr", P, 3e-4), ("seed", P, 42), ("use_roi_if_present", P, True), ("device", P, "cuda"), ("log", P, print), ("plan", P, "host"),
       ("rank", P, 0), ("world_size", P, 1), ("process_group", P, None), ("history", P, None), ("class_weights", P, None),
       ("augment_policy", P, None), ("ema_decay", P, None), ("state_path", P, None), ("resume", P, False), ("init_from", P, None),
       ("freeze_cnn", P, False), ("weight_decay", P, 0.0), ("param_groups", P, None), ("lr_schedule", P, None), ("lr_plateau", P, None),
       ("distill_from", P, None), ("distill_alpha", P, 0.5), ("distill_temperature", P, 2.0)]
TRAINER = [("self", P, NO), ("model", P, NO), ("lr", P, 3e-4), ("max_norm", P, 1.0), ("label_smoothing", P, 0.05),
           ("betas", P, (0.9, 0.999)), ("eps", P, 1e-8), ("world_size", P, 1), ("process_group", P, None), ("dropout", P, True),
           ("micro_batches", P, 1), ("always_allreduce", P, False), ("class_weights", P, None), ("ema_decay", P, None),
           ("ema_warmup", P, True), ("freeze_cnn", P, False), ("weight_decay", P, 0.0), ("param_groups", P, None),
           ("lr_schedule", P, None), ("distill_alpha", P, 0.5), ("distill_temperature", P, 2.0)]
STEP = [("self", P, NO), ("X", P, NO), ("lengths", P, NO), ("R", P, NO), ("y", P, NO), ("global_batch", P, None), ("y_global", P, None),
        ("mix", P, None), ("teacher_logits", P, None)]
STEP_EMBEDDED = [("self", P, NO), ("Z", P, NO), ("lengths", P, NO), ("y", P, NO), ("global_batch", P, None), ("y_global", P, None),
                 ("mix", P, None), ("teacher_logits", P, None)]
FINGERPRINT = [("seed", P, NO), ("batch_size", P, NO), ("world_size", P, NO), ("max_t", P, NO), ("lr", P, NO), ("labels", P, NO),
               ("x_dim", P, NO), ("use_roi", P, NO), ("n_train", P, NO), ("n_val", P, NO), ("class_weights", P, NO),
               ("augment_policy", P, NO), ("ema_decay", P, NO), ("init_from", P, None), ("freeze_cnn", P, False),
               ("weight_decay", P, 0.0), ("param_groups", P, None), ("lr_schedule", P, None), ("lr_plateau", P, None),
               ("distill_from", P, None), ("distill_alpha", P, 0.5), ("distill_temperature", P, 2.0)]
PUBLIC = ["AugmentPolicy", "Config", "BiGRUClassifier", "TinyROICNN", "AttnPool", "Trainer", "allreduce_flat_grads", "shard_range",
          "extract_features", "crop_boxes", "GraphedInference", "load_classifier", "save_checkpoint", "topk_from_logits", "features",
          "data", "checkpoint", "ParamGroup", "no_decay", "LrSchedule", "PlateauSchedule"]


def params(fn):
    return [(p.name, p.kind.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_and_public_names_are_the_written_ones():
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    assert params(Hn.fit) == FIT
    assert params(ss.Trainer.__init__) == TRAINER
    assert params(ss.Trainer.step) == STEP
    assert params(ss.Trainer.step_embedded) == STEP_EMBEDDED
    assert params(Hn.run_fingerprint) == FINGERPRINT
    assert list(ss.__all__) == PUBLIC and all(hasattr(ss, n) for n in PUBLIC)
    # the harness functions other code calls by name
    for name in ("run_fingerprint", "load_init_checkpoint", "check_teacher", "file_sha256", "evaluate", "evaluate_device", "fit"):
        assert callable(getattr(Hn, name)), name
