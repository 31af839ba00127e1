"""The epoch loop with early stopping that the incrementally trained models share (IALSRecommender, SLIM_BPR_Cython): the host mirror
of the reference's Base/Incremental_Training_Early_Stopping.py:93-259.  A class that uses it provides RECOMMENDER_NAME, verbose,
_run_epoch(num_epoch) and _update_best_model(), and may provide _prepare_model_for_validation()."""


class EarlyStoppingMixin(object):
    def _prepare_model_for_validation(self):
        """called in front of every validation: a model whose scores are not read from its training state refreshes them here"""

    def _train_with_early_stopping(self, epochs_max, epochs_min=0, validation_every_n=None, stop_on_validation=False,
                                   validation_metric=None, lower_validations_allowed=None, evaluator_object=None):
        """The training loop of Base/Incremental_Training_Early_Stopping.py:93-259.  Three uses: no evaluator (all epochs, the
        last model is the best one); an evaluator with validation_every_n and validation_metric (all epochs, the model of the best
        validation is kept); and with stop_on_validation and lower_validations_allowed as well (stops once that many validations
        in a row did not improve, not before epoch index epochs_min).  Maintains epochs_best and best_validation_metric."""
        if not epochs_max > 0:
            raise ValueError("{}: Number of epochs_max must be > 0, passed was {}".format(self.RECOMMENDER_NAME, epochs_max))
        if not 0 <= epochs_min <= epochs_max:
            raise ValueError("{}: epochs_min must be in [0, epochs_max], passed are epochs_min {}, epochs_max {}".format(
                self.RECOMMENDER_NAME, epochs_min, epochs_max))
        validating = evaluator_object is not None
        if validating and (validation_every_n is None or validation_metric is None
                           or (stop_on_validation and lower_validations_allowed is None)):
            raise ValueError("{}: Inconsistent parameters passed, please check the supported uses".format(self.RECOMMENDER_NAME))
        self.best_validation_metric = None
        self.epochs_best = 0
        worse_in_a_row = 0
        for epoch in range(epochs_max):
            self._run_epoch(epoch)
            if not validating:
                self.epochs_best = epoch      # (the reference's count without validation: the index of the last epoch)
                continue
            if (epoch + 1) % validation_every_n != 0:
                continue
            self._prepare_model_for_validation()
            results, _ = evaluator_object.evaluateRecommender(self)
            value = results[list(results.keys())[0]][validation_metric]      # several cut-offs: the first one
            if self.best_validation_metric is None or self.best_validation_metric < value:
                self.best_validation_metric = value
                self._update_best_model()
                self.epochs_best = epoch + 1
                worse_in_a_row = 0
            else:
                worse_in_a_row += 1
            if stop_on_validation and worse_in_a_row >= lower_validations_allowed and epoch >= epochs_min:
                if self.verbose:
                    print("{}: Convergence reached! Terminating at epoch {}. Best value for '{}' at epoch {} is {:.4f}".format(
                        self.RECOMMENDER_NAME, epoch + 1, validation_metric, self.epochs_best, self.best_validation_metric))
                break
        if not validating:
            self._update_best_model()

    def get_early_stopping_final_epochs_dict(self):
        return {"epochs": self.epochs_best}
