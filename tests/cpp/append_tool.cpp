// Test driver of add_batch on a searched index through the class surface (tests/test_gpu_append_class.py builds it
// with g++).
//   append_tool d nc code_size centroids info edges pq norm_pq base.fvecs nrounds queries.fvecs nq k nprobe max_codes
//               ef inplace|reupload out.bin out.index
// The reference's add, search, add more, search flow (tests/test_ivfhnsw_grouping_sift1b_vector_add.cpp): the base
// rows go in nrounds consecutive segments (ids = row numbers), each add_batch followed by a search_batch of the
// queries.  reupload calls invalidate_device() after every add_batch, which sends the whole index up again at the next
// search; inplace leaves the class to append on the device.  Writes labels [nrounds][nq][k], then distances in the same
// layout, to out.bin, and the final index to out.index.
#include <ivf-hnsw/IndexIVF_HNSW.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

int main(int argc, char **argv)
try {
    if (argc != 20)
        throw std::runtime_error("usage: see the head of append_tool.cpp");
    const size_t d = atol(argv[1]), nc = atol(argv[2]), cs = atol(argv[3]);
    const char *centroids = argv[4], *info = argv[5], *edges = argv[6], *ppq = argv[7], *pnorm = argv[8],
               *pbase = argv[9];
    const size_t nrounds = atol(argv[10]);
    const char *pqueries = argv[11];
    const size_t nq = atol(argv[12]), k = atol(argv[13]), nprobe = atol(argv[14]), max_codes = atol(argv[15]),
                 ef = atol(argv[16]);
    const std::string mode = argv[17];
    if (mode != "inplace" && mode != "reupload")
        throw std::runtime_error("mode must be inplace or reupload");
    IndexIVF_HNSW *index = new IndexIVF_HNSW(d, nc, cs, 8);
    index->build_quantizer(centroids, info, edges, 16, 500);
    delete index->pq;
    index->pq = faiss::read_ProductQuantizer(ppq);
    delete index->norm_pq;
    index->norm_pq = faiss::read_ProductQuantizer(pnorm);
    index->nprobe = nprobe;
    index->max_codes = max_codes;
    index->quantizer->efSearch = ef;
    std::vector<float> q(nq * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
    }
    std::ifstream bin(pbase, std::ios::binary);
    bin.seekg(0, std::ios::end);
    const size_t nb = (size_t)bin.tellg() / (sizeof(int) + d * sizeof(float));
    bin.seekg(0);
    std::vector<float> base(nb * d);
    readXvec<float>(bin, base.data(), d, nb);
    std::vector<long> lab(nrounds * nq * k);
    std::vector<float> dist(nrounds * nq * k);
    for (size_t r = 0; r < nrounds; r++) {
        const size_t a = nb * r / nrounds, b = nb * (r + 1) / nrounds;
        std::vector<IndexIVF_HNSW::idx_t> ids(b - a);
        for (size_t i = a; i < b; i++)
            ids[i - a] = (IndexIVF_HNSW::idx_t)i;
        index->add_batch(b - a, base.data() + a * d, ids.data());
        if (mode == "reupload")
            index->invalidate_device();
        index->search_batch(nq, k, q.data(), dist.data() + r * nq * k, lab.data() + r * nq * k);
    }
    FILE *f = fopen(argv[18], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    fwrite(lab.data(), sizeof(long), lab.size(), f);
    fwrite(dist.data(), sizeof(float), dist.size(), f);
    fclose(f);
    index->write(argv[19]);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "append_tool: %s\n", e.what());
    return 1;
}
