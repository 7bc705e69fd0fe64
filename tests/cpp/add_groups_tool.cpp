// Test driver of add_group on a searched Grouping index through the class surface (tests/test_gpu_add_groups_class.py
// builds it with g++).
//   add_groups_tool d nc code_size nsubc centroids info edges pq norm_pq base.fvecs assign.u32 nrounds queries.fvecs nq k
//                   nprobe max_codes ef pruning inplace|reupload out.bin out.index
// The reference's vector-add flow (tests/test_ivfhnsw_grouping_sift1b_vector_add.cpp) in rounds: add_group for the next
// nc / nrounds centroids (the rows of base.fvecs whose entry in assign.u32 names the centroid, ids = row numbers; a
// centroid without rows gets an empty group), compute_centroid_norms + compute_inter_centroid_dists, search_batch of the
// queries.  Round 1 searches once more BETWEEN its add_groups and the two table passes.  reupload calls
// invalidate_device() before every search, which sends the whole index up again; inplace leaves the class to add on the
// device.  Writes labels [nrounds + 1][nq][k] (the extra block last), then distances in the same layout, to out.bin, the
// final index to out.index, and prints "full_uploads N".
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

int main(int argc, char **argv)
try {
    if (argc != 23)
        throw std::runtime_error("usage: see the head of add_groups_tool.cpp");
    const size_t d = atol(argv[1]), nc = atol(argv[2]), cs = atol(argv[3]), nsubc = atol(argv[4]);
    const char *centroids = argv[5], *info = argv[6], *edges = argv[7], *ppq = argv[8], *pnorm = argv[9], *pbase = argv[10],
               *passign = argv[11];
    const size_t nrounds = atol(argv[12]);
    const char *pqueries = argv[13];
    const size_t nq = atol(argv[14]), k = atol(argv[15]), nprobe = atol(argv[16]), max_codes = atol(argv[17]),
                 ef = atol(argv[18]);
    const bool pruning = atol(argv[19]) != 0;
    const std::string mode = argv[20];
    if (mode != "inplace" && mode != "reupload")
        throw std::runtime_error("mode must be inplace or reupload");
    IndexIVF_HNSW_Grouping *index = new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
    index->build_quantizer(centroids, info, edges, 16, 500);
    delete index->pq;
    index->pq = faiss::read_ProductQuantizer(ppq);
    delete index->norm_pq;
    index->norm_pq = faiss::read_ProductQuantizer(pnorm);
    index->nprobe = nprobe;
    index->max_codes = max_codes;
    index->do_pruning = pruning;
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
    std::vector<uint32_t> assign(nb);
    {
        std::ifstream in(passign, std::ios::binary);
        in.read(reinterpret_cast<char *>(assign.data()), nb * sizeof(uint32_t));
        if (!in)
            throw std::runtime_error("cannot read the assignment file");
    }
    std::vector<std::vector<size_t>> rows(nc);
    for (size_t i = 0; i < nb; i++)
        rows.at(assign[i]).push_back(i);
    std::vector<long> lab((nrounds + 1) * nq * k, -1);
    std::vector<float> dist((nrounds + 1) * nq * k, 0.f);
    auto search = [&](size_t slot) {
        if (mode == "reupload")
            index->invalidate_device();
        index->search_batch(nq, k, q.data(), dist.data() + slot * nq * k, lab.data() + slot * nq * k);
    };
    for (size_t r = 0; r < nrounds; r++) {
        for (size_t c = nc * r / nrounds; c < nc * (r + 1) / nrounds; c++) {
            std::vector<float> x(rows[c].size() * d);
            std::vector<IndexIVF_HNSW::idx_t> ids(rows[c].size());
            for (size_t j = 0; j < rows[c].size(); j++) {
                std::memcpy(x.data() + j * d, base.data() + rows[c][j] * d, d * sizeof(float));
                ids[j] = (IndexIVF_HNSW::idx_t)rows[c][j];
            }
            index->add_group(c, rows[c].size(), x.data(), ids.data());
        }
        if (r == 1)
            search(nrounds);
        index->compute_centroid_norms();
        index->compute_inter_centroid_dists();
        search(r);
    }
    FILE *f = fopen(argv[21], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    fwrite(lab.data(), sizeof(long), lab.size(), f);
    fwrite(dist.data(), sizeof(float), dist.size(), f);
    fclose(f);
    index->write(argv[22]);
    printf("full_uploads %zu\n", index->device_full_uploads());
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "add_groups_tool: %s\n", e.what());
    return 1;
}
