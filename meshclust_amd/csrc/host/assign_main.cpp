// assign_main.cpp -- bin/meshclust-assign.
#include "assign.hpp"

int main(int argc, char **argv) { return mc::assign_main(argc, argv); }
