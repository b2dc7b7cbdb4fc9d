from ..models.classification import (DecisionTreeClassificationModel, DecisionTreeClassifier,  # noqa: F401
                                     FMClassificationModel, FMClassifier,
                                     GBTClassificationModel, GBTClassifier, LinearSVC, LinearSVCModel,
                                     LogisticRegression, LogisticRegressionModel,
                                     MultilayerPerceptronClassificationModel, MultilayerPerceptronClassifier,
                                     NaiveBayes, NaiveBayesModel,
                                     RandomForestClassificationModel, RandomForestClassifier)
