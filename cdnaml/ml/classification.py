from ..models.classification import (DecisionTreeClassificationModel, DecisionTreeClassifier,  # noqa: F401
                                     GBTClassificationModel, GBTClassifier, LinearSVC, LinearSVCModel,
                                     LogisticRegression, LogisticRegressionModel,
                                     MultilayerPerceptronClassificationModel, MultilayerPerceptronClassifier,
                                     NaiveBayes, NaiveBayesModel,
                                     RandomForestClassificationModel, RandomForestClassifier)
